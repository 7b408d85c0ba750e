"""dm_rssm_sequence_fwd / dm_rssm_sequence_bwd stand-alone through the C-ABI against the fp64 oracle: the body shared by
test_gpu_training_step.py::test_rssm_sequence_fwd_bwd_vs_oracle (Atari-literal cell) and test_gpu_rssm_schedules.py (the
smallest widths that select each launch schedule).  Not a test module.

Oracle = rssm.py:21-78,125-153,186-193 restated in fp64 (oracle.cell_forward / prior_head) with autograd; the loss is a random
projection of (features, post, prior).  make_case() and oracle_run() need no GPU: the per-case seeds of
test_gpu_rssm_schedules.py were chosen with them (free-running oracle, minimum distance of a uniform from an fp64 CDF edge).
"""
import ctypes

import torch
import torch.nn.functional as F

from oracle import dreamer_oracle as O

DEV = 'cuda'
EDGE = 1e-6       # the band around a CDF edge inside which fp32 summation order may legitimately flip a draw


def rel_l2(a, b):
    a, b = a.detach().double().cpu().flatten(), b.detach().double().cpu().flatten()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def max_err(a, b, rtol=0.0):
    """max over elements of |a - b| - rtol |b| (the quantity the absolute bar applies to)"""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float(((a - b).abs() - rtol * b.abs()).max())


def resets_two(T, B, seed):
    """The Atari-literal test's pattern: row 0 at the first step, the last row at step 2."""
    reset = torch.zeros(T, B, dtype=torch.bool)
    reset[0, 0] = True
    reset[min(2, T - 1), B - 1] = True
    return reset


def resets_dense(T, B, seed):
    """A random ~15 % of (t, b), plus one reset at t = 0, plus one row reset at every step (its own generator: the layout of the
    other inputs does not depend on the pattern)."""
    g = torch.Generator().manual_seed(1000 + seed)
    reset = torch.rand(T, B, generator=g) < 0.15
    reset[0, 0] = True
    reset[torch.arange(T), torch.randint(0, B, (T,), generator=g)] = True
    return reset


def make_case(B, T, D_, Hd, S, C, conf_kw=None, resets=resets_two, seed=11, A=18, depth=8, param_seed=4):
    """Config, parameters and inputs of one case (CPU tensors)."""
    oconf = O.make_conf(deter_dim=D_, hidden_dim=Hd, stoch_dim=S, stoch_discrete=C, cnn_depth=depth, action_dim=A,
                        batch_size=B, batch_length=T, **(conf_kw or {}))
    params = O.make_params(oconf, seed=param_seed)
    E, Z, F_ = 32 * depth, S * C, D_ + S * C
    g = torch.Generator().manual_seed(seed)
    c = dict(oconf=oconf, params=params, B=B, T=T, D=D_, Hd=Hd, S=S, C=C, A=A, E=E, Z=Z, F=F_, N=T * B)
    c['embed'] = torch.randn(T, B, E, generator=g)
    c['action'] = F.one_hot(torch.randint(0, A, (T, B), generator=g), A).float()
    c['reset'] = resets(T, B, seed)
    c['h0'] = torch.tanh(torch.randn(B, D_, generator=g))
    c['z0'] = F.one_hot(torch.randint(0, C, (B, S), generator=g), C).float().reshape(B, Z)
    c['u'] = torch.rand(T, B, S, generator=g)
    c['Gf'], c['Gp'], c['Gq'] = (torch.randn(T * B, n, generator=g) / (T * B) for n in (F_, Z, Z))
    return c


def oracle_run(c, forced_idx=None, backward=True):
    """The fp64 oracle over the case's sequence.  forced_idx (T, B, S) or None (free-running: the fp64 draw).  Returns features,
    logits, the draw the fp64 CDF makes along this trajectory, every uniform's distance from the nearest fp64 CDF edge, and
    (backward) the gradients of the random projection."""
    oconf, T, B, S, C, N, Z, F_ = c['oconf'], c['T'], c['B'], c['S'], c['C'], c['N'], c['Z'], c['F']
    pd = {k: v.double().requires_grad_(True) for k, v in c['params'].items() if k.startswith('wm.core.')}
    emb64 = c['embed'].double().requires_grad_(True)
    h, z = c['h0'].double(), c['z0'].double()
    hs, zs, posts, draws, dists = [], [], [], [], []
    for t in range(T):
        mask = (~c['reset'][t]).double().unsqueeze(-1)
        po, h, z, _ = O.cell_forward(pd, oconf, emb64[t], c['action'][t].double(), mask, h, z, c['u'][t].double(),
                                     forced_idx=None if forced_idx is None else forced_idx[t])
        with torch.no_grad():      # what the fp64 CDF draws from these logits, and how far every uniform is from an edge
            cdf = torch.cumsum(torch.softmax(po.detach().reshape(B, S, C), -1), -1)
            target = c['u'][t].double().unsqueeze(-1) * cdf[..., -1:]
            draws.append((cdf <= target).sum(-1).clamp(max=C - 1))
            dists.append((cdf[..., :-1] - target).abs().min(-1).values)      # (the last edge is the clamp, not a decision)
        hs.append(h); zs.append(z); posts.append(po)
    hs, zs, posts = torch.stack(hs), torch.stack(zs), torch.stack(posts)
    priors = O.prior_head(pd, hs)
    out = dict(feat=torch.cat((hs, zs), -1).reshape(N, F_), post=posts.reshape(N, Z), prior=priors.reshape(N, Z),
               draw=torch.stack(draws), dist=torch.stack(dists))
    if backward:
        loss = (out['feat'] * c['Gf'].double()).sum() + (out['post'] * c['Gp'].double()).sum() + (out['prior'] * c['Gq'].double()).sum()
        loss.backward()
        out['grads'] = {k[len('wm.core.cell.'):]: v.grad for k, v in pd.items() if v.grad is not None}
        out['dembed'] = emb64.grad.reshape(N, c['E'])
    return {k: (v.detach() if torch.is_tensor(v) else v) for k, v in out.items()}


def bwd_fold_cut_bytes(c):
    """A backward workspace that ends one 64-float granule short of the folded schedule's buffers: everything BpttCtx::plan
    (csrc/rssm.hip) must have (two split-K scratches, the eight N x Hd and two N x 3D gradient buffers, the five transposed
    weights), then xw2 (N x D), xwz (N x Z), cs2 (D), csz (Z) and the two strip-sum buffers (ceil(Hd / 16) x 128) less one granule."""
    pad = lambda n: (n + 63) // 64 * 64
    N, D_, Hd, Z = c['N'], c['D'], c['Hd'], c['Z']
    splitk = 16 * 1024 * 1024
    must = 2 * splitk + 8 * pad(N * Hd) + 2 * pad(N * 3 * D_) + 2 * pad(Z * Hd) + pad(Hd * D_) + pad(3 * D_ * Hd) + pad(3 * D_ * D_)
    fold = pad(N * D_) + pad(N * Z) + pad(D_) + pad(Z) + 2 * pad((Hd + 15) // 16 * 128)
    return 4 * (must + fold - 64)


def run_case(B, T, D_, Hd, S, C, conf_kw=None, lds=(None,), folds=(None,), resets=resets_two, seed=11, exact_idx=False,
             expect_fwd=None, expect_bwd=None, cut_fold_ws=False, label=None):
    """One shape through dm_rssm_sequence_fwd (once per entry of `lds`: a dm_rssm_lds_enable level, None = leave the switch)
    and dm_rssm_sequence_bwd (once per entry of `folds`: dm_bptt_fold_enable, None = leave; with cut_fold_ws once more on a
    workspace cut below the fold buffers), every run against the fp64 oracle with its indices forced to the first forward's draw.

    expect_fwd(level) / expect_bwd(fold, cut) -> dict of dm_rssm_last_schedule bits that must hold (asserted before any value
    is compared; keys left out are not asserted).
    Bars: features / logits 2e-5 (logits + 1e-5 relative); every parameter gradient and dembed within 2e-4 relative L2.
    Indices: exact_idx - precondition: no uniform within EDGE of an fp64 CDF edge; then ALL equal the fp64 draw.  Otherwise the
    Atari-literal test's bar: > 99.9 % equal.  Switches are restored; dm_rssm_lds_status() == 0 after every call.
    Returns the measured figures (and prints them as one PARITY line per run)."""
    from pydreamer_amd import config, hip as H
    from pydreamer_amd.models import Dreamer
    c = make_case(B, T, D_, Hd, S, C, conf_kw, resets, seed)
    oconf, params, N, E, Z, F_, A = c['oconf'], c['params'], c['N'], c['E'], c['Z'], c['F'], c['A']
    model = Dreamer(config.load_config('defaults', 'atari', **vars(oconf)))
    model.load_state_dict(params, strict=True)
    model = model.to(DEV)
    cell = model.wm.core.cell
    shp = model.wm.shape(T, B, 1)
    ws = model.wm.workspace(shp, torch.device(DEV, 0))
    dev = lambda x: x.to(DEV).contiguous()
    e_d, a_d, r_d, u_d = dev(c['embed'].view(N, E)), dev(c['action'].view(N, A)), dev(c['reset'].view(N).to(torch.uint8)), dev(c['u'].view(N, S))
    # (the initial state stays referenced: a pointer taken from a temporary tensor is handed back to the caching allocator at
    # once, and the next temporary may land on it - round 4 found this test flaky for exactly that reason)
    h0_d, z0_d = dev(c['h0']), dev(c['z0'])
    P = H.rssm_struct(cell.ordered())
    label = label or f'B{B}-T{T}-D{D_}-Hd{Hd}-{S}x{C}'
    lib = H.lib()
    keep_lds, keep_fold = lib.dm_rssm_lds_enable(-1), lib.dm_bptt_fold_enable(-1)
    ora, forced, figures = None, None, []

    def check_bits(which, want, run):
        got = H.last_schedule(which)
        for k, v in (want or {}).items():
            assert got[k] == v, f'{label} {run}: schedule bit {k} is {got[k]}, expected {v} (reported {got})'
        return got

    try:
        for level in lds:
            if level is not None:
                lib.dm_rssm_lds_enable(level)
            acts = torch.empty(int(lib.dm_rssm_acts_floats(ctypes.byref(shp))), device=DEV)
            feat, post, prior = torch.empty(N, F_, device=DEV), torch.empty(N, Z, device=DEV), torch.empty(N, Z, device=DEV)
            idx = torch.empty(N, S, dtype=torch.int32, device=DEV)
            H.call('dm_rssm_sequence_fwd', ctypes.byref(shp), H.fptr(e_d), H.fptr(a_d), H.ptr(r_d), H.fptr(h0_d), H.fptr(z0_d),
                   H.fptr(u_d), None, ctypes.byref(P), H.fptr(acts), H.fptr(feat), H.fptr(post), H.fptr(prior), H.ptr(idx), H.ptr(ws),
                   ws.numel(), H.stream())
            torch.cuda.synchronize()
            assert lib.dm_rssm_lds_status() == 0
            run = f'fwd lds={level}'
            bits = check_bits(0, expect_fwd(level) if expect_fwd else None, run)
            idx_h = idx.cpu().long().view(T, B, S)
            if ora is None:      # oracle, fp64, posterior indices forced to the HIP draw (compared separately below)
                forced, ora = idx_h, oracle_run(c, forced_idx=idx_h)
            same = ora['draw'] == idx_h
            agree, mind = float(same.float().mean()), float(ora['dist'].min())
            fig = dict(run=run, bits=bits, idx_agree=agree, min_edge_dist=mind, feat=max_err(feat, ora['feat']),
                       post=max_err(post, ora['post'], 1e-5), prior=max_err(prior, ora['prior'], 1e-5))
            print(f"PARITY {label} {run} bits={_fmt(bits)} idx_equal={agree:.6f} min_edge_dist={mind:.2e} feat={fig['feat']:.2e} "
                  f"post={fig['post']:.2e} prior={fig['prior']:.2e}")
            figures.append(fig)
            if exact_idx:
                assert mind >= EDGE, f'{label}: precondition - a uniform lies {mind:.2e} from an fp64 CDF edge (choose another seed)'
                assert bool(same.all()), f'{label} {run}: {int((~same).sum())} of {same.numel()} indices differ from the fp64 draw'
            else:
                print('index agreement with the oracle per step:', same.float().mean(dim=(1, 2)).tolist(),
                      'per row:', same.float().mean(dim=(0, 2)).tolist())
                assert agree > 0.999, agree
            assert torch.equal(idx_h, forced), f'{label} {run}: draw differs from the first forward run'
            assert fig['feat'] <= 2e-5, (label, run, 'rssm features', fig['feat'])
            assert fig['post'] <= 2e-5, (label, run, 'rssm post logits', fig['post'])
            assert fig['prior'] <= 2e-5, (label, run, 'rssm prior logits', fig['prior'])
        names = H.rssm_param_names(oconf.gru_type, oconf.gru_layers)
        bwd_runs = [(f, False) for f in folds] + ([(1, True)] if cut_fold_ws else [])
        for fold, cut in bwd_runs:
            if fold is not None:
                lib.dm_bptt_fold_enable(fold)
            ws_bytes = ws.numel()
            if cut:
                ws_bytes = bwd_fold_cut_bytes(c)
                assert ws_bytes <= ws.numel(), (ws_bytes, ws.numel())
            grads = [None if p_ is None else torch.zeros_like(p_) for p_ in cell.ordered()]
            Gs = H.rssm_struct(grads, cls=H.dm_rssm_grads)
            dembed = torch.empty(N, E, device=DEV)
            dfeat, dpost, dprior = dev(c['Gf']), dev(c['Gp']), dev(c['Gq'])
            H.call('dm_rssm_sequence_bwd', ctypes.byref(shp), H.fptr(e_d), H.fptr(a_d), H.ptr(r_d), ctypes.byref(P), H.fptr(acts),
                   H.fptr(feat), H.fptr(post), H.fptr(dfeat), H.fptr(dpost), H.fptr(dprior), ctypes.byref(Gs), H.fptr(dembed),
                   H.ptr(ws), ws_bytes, H.stream())
            torch.cuda.synchronize()
            assert lib.dm_rssm_lds_status() == 0
            run = f'bwd fold={fold}' + (' cut-ws' if cut else '')
            bits = check_bits(1, expect_bwd(fold, cut) if expect_bwd else None, run)
            errs = {name: rel_l2(gh, ora['grads'][name]) for name, gh in zip(names, grads) if name is not None and gh is not None}
            errs['dembed'] = rel_l2(dembed, ora['dembed'])
            worst = max(errs, key=errs.get)
            print(f'PARITY {label} {run} bits={_fmt(bits)} worst_grad_rel_l2={errs[worst]:.2e} at {worst}')
            figures.append(dict(run=run, bits=bits, worst=worst, worst_err=errs[worst]))
            for name, e in errs.items():
                assert e < 2e-4, (label, run, name, e)
    finally:
        lib.dm_rssm_lds_enable(keep_lds)
        lib.dm_bptt_fold_enable(keep_fold)
    return figures


def run_on_own_parts(B, T, D_, Hd, S, C, expect_fwd, expect_bwd, seed=11, lds_level=2):
    """dm_rssm_sequence_fwd (at dm_rssm_lds_enable `lds_level`) and dm_rssm_sequence_bwd twice: on dm_workspace_bytes, and each
    on a workspace of exactly its own part of dm_workspace_query.  Both runs must report the schedule bits expect_fwd /
    expect_bwd - asserted before any value is looked at - and then give the same bits in every output and gradient."""
    from pydreamer_amd import config, hip as H
    from pydreamer_amd.models import Dreamer
    c = make_case(B, T, D_, Hd, S, C, None, resets_dense, seed)
    oconf, N, E, Z, F_, A = c['oconf'], c['N'], c['E'], c['Z'], c['F'], c['A']
    model = Dreamer(config.load_config('defaults', 'atari', **vars(oconf)))
    model.load_state_dict(c['params'], strict=True)
    model = model.to(DEV)
    cell = model.wm.core.cell
    shp = model.wm.shape(T, B, 1)
    parts = (ctypes.c_size_t * 8)()
    H.call('dm_workspace_query', ctypes.byref(shp), parts, 8)
    sizes = {'full': (H.workspace_bytes(shp),) * 2, 'own': (4 * int(parts[4]), 4 * int(parts[5]))}
    assert max(sizes['own']) < sizes['full'][0]
    dev = lambda x: x.to(DEV).contiguous()
    e_d, a_d, r_d, u_d = dev(c['embed'].view(N, E)), dev(c['action'].view(N, A)), dev(c['reset'].view(N).to(torch.uint8)), dev(c['u'].view(N, S))
    h0_d, z0_d = dev(c['h0']), dev(c['z0'])
    P = H.rssm_struct(cell.ordered())
    lib = H.lib()
    keep_lds = lib.dm_rssm_lds_enable(-1)
    out = {}
    try:
        lib.dm_rssm_lds_enable(lds_level)
        for tag, (fwd_bytes, bwd_bytes) in sizes.items():
            ws_f = torch.empty(fwd_bytes, dtype=torch.uint8, device=DEV)
            ws_b = torch.empty(bwd_bytes, dtype=torch.uint8, device=DEV)
            acts = torch.empty(int(lib.dm_rssm_acts_floats(ctypes.byref(shp))), device=DEV)
            feat, post, prior = torch.empty(N, F_, device=DEV), torch.empty(N, Z, device=DEV), torch.empty(N, Z, device=DEV)
            idx = torch.empty(N, S, dtype=torch.int32, device=DEV)
            H.call('dm_rssm_sequence_fwd', ctypes.byref(shp), H.fptr(e_d), H.fptr(a_d), H.ptr(r_d), H.fptr(h0_d), H.fptr(z0_d),
                   H.fptr(u_d), None, ctypes.byref(P), H.fptr(acts), H.fptr(feat), H.fptr(post), H.fptr(prior), H.ptr(idx),
                   H.ptr(ws_f), fwd_bytes, H.stream())
            torch.cuda.synchronize()
            assert lib.dm_rssm_lds_status() == 0
            got = H.last_schedule(0)
            print(f'SCHEDULE {tag} fwd ({fwd_bytes} bytes) {_fmt(got)}')
            for k, v in expect_fwd.items():
                assert got[k] == v, f'{tag} forward workspace ({fwd_bytes} bytes): schedule bit {k} is {got[k]}, expected {v} ({got})'
            grads = [None if p_ is None else torch.zeros_like(p_) for p_ in cell.ordered()]
            Gs = H.rssm_struct(grads, cls=H.dm_rssm_grads)
            dembed = torch.empty(N, E, device=DEV)
            dfeat, dpost, dprior = dev(c['Gf']), dev(c['Gp']), dev(c['Gq'])
            H.call('dm_rssm_sequence_bwd', ctypes.byref(shp), H.fptr(e_d), H.fptr(a_d), H.ptr(r_d), ctypes.byref(P), H.fptr(acts),
                   H.fptr(feat), H.fptr(post), H.fptr(dfeat), H.fptr(dpost), H.fptr(dprior), ctypes.byref(Gs), H.fptr(dembed),
                   H.ptr(ws_b), bwd_bytes, H.stream())
            torch.cuda.synchronize()
            got = H.last_schedule(1)
            print(f'SCHEDULE {tag} bwd ({bwd_bytes} bytes) {_fmt(got)}')
            for k, v in expect_bwd.items():
                assert got[k] == v, f'{tag} backward workspace ({bwd_bytes} bytes): schedule bit {k} is {got[k]}, expected {v} ({got})'
            out[tag] = dict(feat=feat, post=post, prior=prior, idx=idx, dembed=dembed, dfeat=dfeat, dpost=dpost,
                            **{f'grad {i}': g for i, g in enumerate(grads) if g is not None})
    finally:
        lib.dm_rssm_lds_enable(keep_lds)
    assert all(bool(torch.isfinite(v).all()) for v in out['own'].values() if v.is_floating_point())
    differ = [k for k in out['full'] if not torch.equal(out['full'][k].view(torch.int32), out['own'][k].view(torch.int32))]
    assert not differ, f'{differ} differ between workspaces of the calls\' own parts and dm_workspace_bytes'


def _fmt(bits):
    on = [k for k, v in bits.items() if v is True]
    return '+'.join(on + ([f"nchunk{bits['nchunk']}"] if 'nchunk' in bits else [])) or 'none'
