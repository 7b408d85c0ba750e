"""-m gpu: the convolution stack (dm_conv_encoder_fwd / _bwd, dm_conv_decoder_mse_fwd / _bwd_rows) through the C-ABI, EVERY
element of EVERY output against the fp64 CPU oracle, at the frame counts the trainer runs (2 500 = Atari-literal 50 x 50,
1 536 = Atari-native 32 x 48), around the 512-workgroup cap of the direct kernels, at ragged M, at every depth the direct
kernels take and at shapes they refuse (explicit patch matrix, scalar / 4-wide gather tables, col2im data gradient).

What is compared (nothing sampled): encoder `embed`, dW / db of its 4 layers; decoder `image_rec`, `loss_image`, the NHWC
prediction inside `acts` at dm_conv_decoder_pred_offset, `dfeat` (accumulated onto previous content of its own magnitude,
lddf > F, columns beyond F untouched), dW / db of its 5 layers.

Metric per tensor: err = max_i |got_i - ref64_i| / rms(ref64) (oracle/conv_reference.py).  One wrong element of ordinary
size gives err ~ 1 however many million terms the tensor has; a relative L2 norm over the tensor hides it.
Bar per tensor, computed at run time: max(10 * err_ref32, 64 * eps_fp32), where err_ref32 is the same metric of the SAME oracle
functions run in fp32 on the CPU on the same inputs.  Ten is this suite's convention (the full-size step test keeps its bars
at ~10x the measured values) and covers what legitimately differs between two fp32 evaluations: tile / split-K order here,
frame-by-frame accumulation in torch.  The floor (7.6e-6) is for short sums that the CPU happens to get almost exactly.

Out-of-bounds writes: every buffer the library writes is a slice of a larger allocation whose 16 KiB before and after it
hold a NaN bit pattern (0x7FC5A5A5), compared bit for bit after the calls; `acts` and the workspace are sized exactly to
dm_conv_*_acts_floats / dm_workspace_bytes and are pre-filled with the same NaNs, so a kernel that reads scratch it never wrote
shows up as a non-finite result.  `feat` is a slice (ldf > F) of a matrix whose other columns are NaN.

Inputs come from seeds: frames are uint8 (N, 64, 64, C) bytes; the float path gets fp32(x / 255 - 0.5) of them, the uint8 path
(DM_FLAG_IMAGE_U8) the bytes themselves; the fp64 reference takes x / 255 - 0.5 of the bytes in fp64, the fp32 CPU run in fp32, so
one cached reference per (depth, channels, frames, seed) serves the float, uint8, layer-4-switch and side-stream variants.

Cases (T = 1, B = frames):
  depth 48, 3 channels: 2500, 1536 (production); 1, 511, 512, 513, 1025 (direct kernels' 512-workgroup cap); 67, 131 (ragged M)
  depth 8, 16, 32, 64, 3 channels: 131; depth 32 also 513
  depth 24, 12, 6, 3 channels: 131 - no direct kernels: explicit layer-1 patch matrix, column-matrix image layer; depth 12 has
      cin % 8 != 0 (4-wide gather), depth 6 has cin % 4 != 0 (scalar gather) and cout < 16 (col2im data gradient)
  depth 48 and 8, 1 channel: 131 - explicit patch matrix with K = 16, image layer with 1 -> 4 padded channels
  variants on depth 48 at 2500 and 131 frames: uint8 frames; dm_conv_decoder_mse_bwd_rows with a non-constant row_scale;
      I = 3 with row_scale (frames = B * 3: 2499 = 833 * 3 and 129 = 43 * 3, since neither 2500 nor 131 is a multiple of 3);
      dm_dec_l4_bwd_direct_enable(0 / 1); dm_wgrad_side_arm ... _join (bit-identical to the unarmed call).
  No shape of this table is refused by the library (DM_E_SHAPE); all of them compute.  Depth 6 is the case this module found
  wrong when it was written: a decoder layer whose channel count is not a multiple of 4 (6) takes its output gradient at a
  padded pitch (8), and the layer above wrote it at the unpadded one - every decoder gradient below the image layer was off by
  err ~ 10.  Fixed in conv_decoder_mse_bwd_impl (csrc/conv.hip).

Measured on the MI355X (depth 48, 3 channels, 2 500 frames; err_ref32 as measured on the test host's CPU, then the ratio
err / err_ref32 of the float path and of each variant; the bar is at ratio 10).  uint8 frames give the float path's values bit for bit.
  tensor                err_ref32   float   _bwd_rows   I = 3 (2 499)   image-layer backward as products
  encoder embed          3.0e-06     2.46
  encoder dW0 / db0      5.7e-06 / 4.3e-06   0.55 / 0.50
  encoder dW1 / db1      5.9e-06 / 3.4e-06   1.20 / 0.42
  encoder dW2 / db2      5.8e-06 / 2.1e-06   1.22 / 0.81
  encoder dW3 / db3      3.4e-06 / 1.1e-06   1.96 / 0.61
  decoder image_rec      4.7e-06     1.48     1.48        1.53            1.48      (the prediction inside `acts`: the same values)
  decoder loss_image     2.1e-07     1.01     1.01        0.94            1.01      (bar = the floor)
  decoder dfeat (+prev)  2.4e-06     1.93     2.04        1.92            2.03
  decoder dW0 / db0      2.8e-06 / 1.4e-06   2.45 / 1.25   2.13 / 1.13   1.81 / 1.24   2.09 / 1.32
  decoder dW1 / db1      3.8e-06 / 1.2e-06   3.40 / 0.94   4.93 / 0.72   3.66 / 0.84   3.26 / 0.90
  decoder dW2 / db2      2.8e-06 / 2.4e-06   1.27 / 0.43   1.50 / 0.50   1.21 / 0.46   1.55 / 0.44
  decoder dW3 / db3      3.0e-06 / 5.2e-06   1.26 / 0.19   1.11 / 0.48   1.33 / 0.34   1.12 / 0.19
  decoder dW4 / db4      1.4e-06 / 5.4e-07   0.64 / 0.96   0.74 / 1.00   0.59 / 1.07   2.78 / 0.96
Worst ratio over all 31 tests of the module: 4.93 (decoder dW1, _bwd_rows at 2 500 frames).  Wall time of the module on the MI355X
host with 16 CPU threads: 2.1 minutes, of which 104 s are the CPU references.
"""
import ctypes
import time

import pytest
import torch

from oracle import conv_reference as R
from oracle import dreamer_oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SEED = 11
GUARD = 4096                 # canary elements (16 KiB) on each side of every buffer the library writes
CANARY = 0x7FC5A5A5          # a quiet NaN with a payload, as int32
PINNED = {(48, 3, 2500), (48, 3, 131)}      # references shared by the variants; every other one is computed, used and dropped


# ------------------------------------------------------------------------------------------------ buffers with canaries
class Guarded:
    """`numel` 4-byte elements between two canary regions; the interior starts out as the canary pattern too."""

    def __init__(self, name, numel, book):
        self.name, self.numel = name, int(numel)
        self.raw = torch.full((self.numel + 2 * GUARD,), CANARY, dtype=torch.int32, device=DEV)
        self.t = self.raw[GUARD:GUARD + self.numel].view(torch.float32)
        book.append(self)

    def damage(self):
        head, tail = self.raw[:GUARD], self.raw[GUARD + self.numel:]
        bad = [(side, int((part != CANARY).sum()), int((part != CANARY).nonzero()[0]))
               for side, part in (('before', head), ('after', tail)) if bool((part != CANARY).any())]
        return bad


def _assert_canaries(book, what):
    torch.cuda.synchronize()
    for b in book:
        bad = b.damage()
        assert not bad, f'{what}: out-of-bounds write around `{b.name}` ({b.numel} elements): ' + '; '.join(
            f'{n} canary words changed {side} it, first at offset {first}' for side, n, first in bad)


# ------------------------------------------------------------------------------------------------ inputs and references
def _hip_conf(oconf):
    from pydreamer_amd import config
    return config.load_config('defaults', 'atari', **{k: getattr(oconf, k) for k in vars(oconf)})


_MODELS = {}


def _model(depth, ch):
    if (depth, ch) not in _MODELS:
        from pydreamer_amd.models import Dreamer
        oconf = O.tiny_conf(cnn_depth=depth, image_channels=ch)
        params = O.make_params(oconf)
        model = Dreamer(_hip_conf(oconf))
        model.load_state_dict(params, strict=True)
        _MODELS[(depth, ch)] = (oconf, params, model.to(DEV))
    return _MODELS[(depth, ch)]


def _inputs(oconf, frames, seed=SEED):
    g = torch.Generator().manual_seed(seed * 1000003 + frames)
    ch = oconf.image_channels
    raw = torch.randint(0, 256, (frames, 64, 64, ch), generator=g, dtype=torch.uint8)
    return dict(raw=raw, image=(raw.float() / 255.0 - 0.5).permute(0, 3, 1, 2).contiguous(),
                feat=torch.randn(frames, O.feature_dim(oconf), generator=g),
                dembed=torch.randn(frames, 32 * oconf.cnn_depth, generator=g),
                row_scale=0.25 + 1.5 * torch.rand(frames, generator=g))


def _scale(frames):
    return 1.0 / frames          # the trainer's image_weight / (T * B)


class _Refs:
    """fp64 and fp32 CPU references per (depth, channels, frames): {'inp', 'enc64', 'enc32', 'dec64', 'dec32'}."""

    def __init__(self):
        self.kept = {}
        self.seconds = 0.0

    def get(self, depth, ch, frames, encoder=True, decoder=True):
        key = (depth, ch, frames)
        if key in self.kept:
            return self.kept[key]
        oconf, params, _ = _model(depth, ch)
        inp = _inputs(oconf, frames)
        t0 = time.time()
        ref = dict(inp=inp)
        for tag, dt in (('64', torch.float64), ('32', torch.float32)):
            if encoder:
                ref['enc' + tag] = R.encoder_reference(params, inp['raw'], inp['dembed'], dtype=dt)
            if decoder:
                ref['dec' + tag] = R.decoder_reference(params, inp['feat'], inp['raw'], _scale(frames), dtype=dt)
        self.seconds += time.time() - t0
        print(f'[reference] depth {depth} channels {ch} frames {frames}: {time.time() - t0:.1f} s (total {self.seconds:.1f} s)')
        if key in PINNED:
            self.kept[key] = ref
        return ref


@pytest.fixture(scope='module')
def refs():
    r = _Refs()
    yield r
    print(f'[reference] CPU reference time of this module: {r.seconds:.1f} s')
    _MODELS.clear()


# ------------------------------------------------------------------------------------------------ the calls
def _shape(model, frames, I=1, flags=0):
    shp = model.wm.shape(1, frames // I, 1)
    shp.I = I
    shp.flags |= flags
    return shp


def _workspace(H, shp, book, floats=None):
    """dm_workspace_bytes of canary-fenced scratch, or exactly `floats` floats"""
    nbytes = H.workspace_bytes(shp) if floats is None else 4 * floats
    assert nbytes % 4 == 0
    ws = Guarded('workspace', nbytes // 4, book)
    return ws, ctypes.c_void_p(ws.t.data_ptr()), nbytes


def _run_encoder(H, model, frames, inp, u8=False, flags=0, bwd_floats=None, bwd_cut=0, book=None):
    """dm_conv_encoder_fwd + _bwd.  Returns the outputs in the reference's layouts (on the CPU).  bwd_floats: the backward runs
    on a workspace of its own of exactly that many floats, and is told it has bwd_cut bytes less; book: the caller's list of the
    buffers."""
    shp = _shape(model, frames, flags=flags | (H.DM_FLAG_IMAGE_U8 if u8 else 0))
    enc = model.wm.encoder.encoder_image
    E = enc.out_dim
    book = [] if book is None else book
    ws, ws_p, ws_n = _workspace(H, shp, book)
    acts = Guarded('encoder acts', int(H.lib().dm_conv_encoder_acts_floats(ctypes.byref(shp))), book)
    embed = Guarded('embed', frames * E, book)
    gw = [Guarded(f'encoder dW{i}', m.weight.numel(), book) for i, m in enumerate(enc.convs())]
    gb = [Guarded(f'encoder db{i}', m.bias.numel(), book) for i, m in enumerate(enc.convs())]
    image = (inp['raw'] if u8 else inp['image']).to(DEV)
    dembed = inp['dembed'].to(DEV)
    enc_p = H.conv_struct([m.weight for m in enc.convs()], [m.bias for m in enc.convs()])
    enc_g = H.conv_struct([g.t for g in gw], [g.t for g in gb], cls=H.dm_conv_grads)
    H.call('dm_conv_encoder_fwd', ctypes.byref(shp), H.ptr(image), ctypes.byref(enc_p), H.fptr(acts.t), H.fptr(embed.t), ws_p, ws_n,
           H.stream())
    if bwd_floats is not None:
        ws, ws_p, ws_n = _workspace(H, shp, book, bwd_floats)
    H.call('dm_conv_encoder_bwd', ctypes.byref(shp), H.ptr(image), ctypes.byref(enc_p), H.fptr(acts.t), H.fptr(dembed),
           ctypes.byref(enc_g), ws_p, ws_n - bwd_cut, H.stream())
    _assert_canaries(book, f'encoder, {frames} frames')
    out = {'embed': embed.t.view(frames, E).cpu()}
    for i, m in enumerate(enc.convs()):
        out[f'dW{i}'] = gw[i].t.view_as(m.weight).cpu()
        out[f'db{i}'] = gb[i].t.view_as(m.bias).cpu()
    return out


def _run_decoder(H, model, frames, inp, u8=False, I=1, row_scale=None, side=False, dfeat_prev=None, pad_f=8, pad_df=12, flags=0,
                 fwd_floats=None, bwd_floats=None, fwd_cut=0, bwd_cut=0, book=None):
    """dm_conv_decoder_mse_fwd + dm_conv_decoder_mse_bwd_rows.  feat is an ldf = F + pad_f slice of a NaN-filled matrix, dfeat an
    lddf = F + pad_df slice holding `dfeat_prev` (all columns).  side: the backward runs armed (dm_wgrad_side_arm ... _join) on a
    workspace nothing else touches before the join.  fwd_floats / bwd_floats: that call runs on a workspace of exactly that
    many floats, and is told it has fwd_cut / bwd_cut bytes less; book: the caller's list of the buffers."""
    shp = _shape(model, frames, I=I, flags=flags | (H.DM_FLAG_IMAGE_U8 if u8 else 0))
    dl = model.wm.decoder.image.layers()
    F_, ch = model.wm.features_dim, model.conf.image_channels
    ldf, lddf = F_ + pad_f, F_ + pad_df
    book = [] if book is None else book
    ws, ws_p, ws_n = _workspace(H, shp, book, fwd_floats)
    acts = Guarded('decoder acts', int(H.lib().dm_conv_decoder_acts_floats(ctypes.byref(shp))), book)
    loss = Guarded('loss_image', frames, book)
    rec = Guarded('image_rec', frames * ch * 4096, book)
    gw = [Guarded(f'decoder dW{i}', m.weight.numel(), book) for i, m in enumerate(dl)]
    gb = [Guarded(f'decoder db{i}', m.bias.numel(), book) for i, m in enumerate(dl)]
    dfeat = Guarded('dfeat', frames * lddf, book)
    featm = torch.full((frames, ldf), float('nan'), device=DEV)
    featm[:, :F_] = inp['feat'].to(DEV)
    prev = torch.randn(frames, lddf, generator=torch.Generator().manual_seed(SEED + 1)) if dfeat_prev is None else dfeat_prev
    dfeat.t.view(frames, lddf).copy_(prev.to(DEV))
    target = (inp['raw'] if u8 else inp['image'])[:frames // I].contiguous().to(DEV)
    rs = None if row_scale is None else row_scale.to(DEV)
    dec_p = H.conv_struct([m.weight for m in dl], [m.bias for m in dl])
    dec_g = H.conv_struct([g.t for g in gw], [g.t for g in gb], cls=H.dm_conv_grads)
    H.call('dm_conv_decoder_mse_fwd', ctypes.byref(shp), H.fptr(featm), ldf, H.ptr(target), ctypes.byref(dec_p), H.fptr(acts.t),
           H.fptr(loss.t), H.fptr(rec.t), ws_p, ws_n - fwd_cut, H.stream())
    if bwd_floats is not None:
        ws, ws_p, ws_n = _workspace(H, shp, book, bwd_floats)
    if side:
        H.call('dm_wgrad_side_arm', 1)
    try:
        H.call('dm_conv_decoder_mse_bwd_rows', ctypes.byref(shp), H.fptr(featm), ldf, H.ptr(target), ctypes.byref(dec_p),
               H.fptr(acts.t), _scale(frames), H.fptr(rs), ctypes.byref(dec_g), H.fptr(dfeat.t), lddf, ws_p, ws_n - bwd_cut,
               H.stream())
    finally:
        if side:
            H.call('dm_wgrad_side_join', H.stream())
    _assert_canaries(book, f'decoder, {frames} frames')
    off = int(H.lib().dm_conv_decoder_pred_offset(ctypes.byref(shp)))
    assert off + frames * 4096 * ch <= acts.numel
    out = {'image_rec': rec.t.view(frames, ch, 64, 64).cpu(), 'loss_image': loss.t.cpu(),
           'pred_nhwc': acts.t[off:off + frames * 4096 * ch].view(frames, 64, 64, ch).cpu(),
           'dfeat_full': dfeat.t.view(frames, lddf).cpu(), 'dfeat_prev': prev}
    for i, m in enumerate(dl):
        out[f'dW{i}'] = gw[i].t.view_as(m.weight).cpu()
        out[f'db{i}'] = gb[i].t.view_as(m.bias).cpu()
    return out


# ------------------------------------------------------------------------------------------------ the comparison
W_AXES = ('out', 'in', 'ky', 'kx')
WT_AXES = ('in', 'out', 'ky', 'kx')        # ConvTranspose2d weights


def _print_report(title, report):
    print(f'\n[{title}]')
    for name, err, err32, bar in report:
        print(f'  {name:<22} err {err:.3e}  err_ref32 {err32:.3e}  err/err_ref32 {err / max(err32, 1e-300):7.2f}  bar {bar:.3e}')


def _check_all(title, checks):
    """checks: (name, got, ref64, ref32, axes).  Every tensor is measured and printed before the first failure is raised."""
    report, failures = [], []
    for name, got, r64, r32, axes in checks:
        try:
            R.check_tensor(name, got, r64, r32, axes, report)
        except AssertionError as e:
            failures.append(str(e))
    _print_report(title, report)
    assert not failures, f'{title}: ' + ' | '.join(failures)
    return report


def _encoder_checks(out, ref):
    r64, r32 = ref['enc64'], ref['enc32']
    checks = [('encoder embed', out['embed'], r64['embed'], r32['embed'], ('frame', 'feature(c,y,x)'))]
    for i in range(4):
        checks.append((f'encoder dW{i}', out[f'dW{i}'], r64[f'dW{i}'], r32[f'dW{i}'], W_AXES))
        checks.append((f'encoder db{i}', out[f'db{i}'], r64[f'db{i}'], r32[f'db{i}'], ('out',)))
    return checks


def dfeat_prev_for(ref64_dfeat, lddf):
    """Previous content of the dfeat buffer: random, of the gradient's own magnitude (onto ones, a 1e-4-sized gradient would
    vanish in the rounding of the sum and the comparison would prove nothing)."""
    rms = float(ref64_dfeat.square().mean().sqrt())
    return (torch.randn(ref64_dfeat.shape[0], lddf, generator=torch.Generator().manual_seed(SEED + 2)) * rms).float()


def _decoder_checks(out, r64, r32, F_):
    prev = out['dfeat_prev']
    got = out['dfeat_full']
    assert torch.equal(got[:, F_:].view(torch.int32), prev[:, F_:].view(torch.int32)), 'dfeat: columns beyond F were written'
    # the accumulate is part of what is judged: reference = previous content + gradient, in fp64 and (for the bar) in fp32
    tot64 = prev[:, :F_].double() + r64['dfeat']
    tot32 = prev[:, :F_] + r32['dfeat']
    checks = [('decoder image_rec', out['image_rec'], r64['image_rec'], r32['image_rec'], ('frame', 'channel', 'y', 'x')),
              ('decoder pred (acts)', out['pred_nhwc'], r64['image_rec'].permute(0, 2, 3, 1), r32['image_rec'].permute(0, 2, 3, 1),
               ('frame', 'y', 'x', 'channel')),
              ('decoder loss_image', out['loss_image'], r64['loss_image'], r32['loss_image'], ('frame',)),
              ('decoder dfeat(+prev)', got[:, :F_], tot64, tot32, ('frame', 'feature'))]
    for i in range(5):
        checks.append((f'decoder dW{i}', out[f'dW{i}'], r64[f'dW{i}'], r32[f'dW{i}'], ('out', 'in') if i == 0 else WT_AXES))
        checks.append((f'decoder db{i}', out[f'db{i}'], r64[f'db{i}'], r32[f'db{i}'], ('out',)))
    return checks


def _decoder_case(H, model, frames, ref, title, **kw):
    F_ = model.wm.features_dim
    prev = dfeat_prev_for(ref['dec64']['dfeat'], F_ + 12)
    out = _run_decoder(H, model, frames, ref['inp'], dfeat_prev=prev, **kw)
    return _check_all(title, _decoder_checks(out, ref['dec64'], ref['dec32'], F_))


# ------------------------------------------------------------------------------------------------ the cases
CASES = ([(48, 3, n) for n in (2500, 1536, 1, 511, 512, 513, 1025, 67, 131)] +
         [(8, 3, 131), (16, 3, 131), (32, 3, 131), (32, 3, 513), (64, 3, 131)] +
         [(24, 3, 131), (12, 3, 131), (6, 3, 131)] +
         [(48, 1, 131), (8, 1, 131)])


@pytest.mark.parametrize('depth,ch,frames', CASES, ids=[f'd{d}-c{c}-n{n}' for d, c, n in CASES])
def test_conv_stack_every_element(hip, refs, depth, ch, frames):
    """Encoder and decoder forward + backward, float frames, the library's default switches."""
    _, _, model = _model(depth, ch)
    ref = refs.get(depth, ch, frames)
    failures = []
    for part in (lambda: _check_all(f'encoder depth {depth} channels {ch} frames {frames}',
                                    _encoder_checks(_run_encoder(hip, model, frames, ref['inp']), ref)),
                 lambda: _decoder_case(hip, model, frames, ref, f'decoder depth {depth} channels {ch} frames {frames}')):
        try:      # a wrong encoder tensor does not hide what the decoder does at this shape
            part()
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, ' || '.join(failures)


@pytest.mark.parametrize('frames', [2500, 131])
def test_uint8_frames(hip, refs, frames):
    """DM_FLAG_IMAGE_U8: the encoder input and the decoder target are the replay's bytes; same reference (x / 255 - 0.5 of them)."""
    _, _, model = _model(48, 3)
    ref = refs.get(48, 3, frames)
    out = _run_encoder(hip, model, frames, ref['inp'], u8=True)
    _check_all(f'encoder uint8 frames {frames}', _encoder_checks(out, ref))
    _decoder_case(hip, model, frames, ref, f'decoder uint8 frames {frames}', u8=True)


@pytest.mark.parametrize('frames,I', [(2500, 1), (131, 1), (2499, 3), (129, 3)])
def test_decoder_bwd_rows_row_scale_and_iwae(hip, refs, frames, I):
    """dm_conv_decoder_mse_bwd_rows as the trainer calls it: a per-frame factor on the loss gradient, and I = 3 (frames = B * I,
    prediction frame n against target frame n // I).  Reference: the same oracle, target repeated, per-frame loss weighted."""
    oconf, params, model = _model(48, 3)
    inp = _inputs(oconf, frames) if I > 1 else refs.get(48, 3, frames)['inp']
    t0 = time.time()
    r64, r32 = (R.decoder_reference(params, inp['feat'], inp['raw'][:frames // I], _scale(frames), row_scale=inp['row_scale'], tdiv=I,
                                    dtype=dt) for dt in (torch.float64, torch.float32))
    refs.seconds += time.time() - t0
    F_ = model.wm.features_dim
    out = _run_decoder(hip, model, frames, inp, I=I, row_scale=inp['row_scale'], dfeat_prev=dfeat_prev_for(r64['dfeat'], F_ + 12))
    _check_all(f'decoder _bwd_rows frames {frames} I {I}', _decoder_checks(out, r64, r32, F_))


@pytest.mark.parametrize('frames,l4_direct', [(2500, 0), (2500, 1), (131, 0), (131, 1)])
def test_decoder_image_layer_backward_switch(hip, refs, frames, l4_direct):
    """dm_dec_l4_bwd_direct_enable: the image layer's backward as the two direct kernels (1) or as gather-form products (0)."""
    _, _, model = _model(48, 3)
    ref = refs.get(48, 3, frames)
    before = hip.lib().dm_dec_l4_bwd_direct_enable(-1)
    hip.lib().dm_dec_l4_bwd_direct_enable(l4_direct)
    try:
        _decoder_case(hip, model, frames, ref, f'decoder frames {frames} l4 backward direct {l4_direct}')
    finally:
        hip.lib().dm_dec_l4_bwd_direct_enable(before)


def test_decoder_backward_on_the_side_stream_is_bit_identical(hip):
    """dm_wgrad_side_arm(1) ... dm_wgrad_side_join around the decoder backward at 2 500 frames: every gradient bit-identical to the
    unarmed call (same kernels, same arguments, another stream).  The armed call's workspace is its own until the join."""
    oconf, _, model = _model(48, 3)
    inp = _inputs(oconf, 2500)
    a = _run_decoder(hip, model, 2500, inp, row_scale=inp['row_scale'])
    b = _run_decoder(hip, model, 2500, inp, row_scale=inp['row_scale'], side=True)
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), f'{k} differs between the armed and the unarmed call'
    assert torch.isfinite(a['dW4']).all() and torch.isfinite(a['dfeat_full'][:, :model.wm.features_dim]).all()


# ------------------------------------------------------------------------------------------------ did it reach what it claims
TILES = ('128x128', '128x64', '64x64', '128x96', '96x128')


def _profiled_rows(H, model, frames, inp):
    cap = 512
    H.call('dm_prof_begin', cap)
    try:
        _run_encoder(H, model, frames, inp)
        _run_decoder(H, model, frames, inp)
        torch.cuda.synchronize()
        rows = (ctypes.c_double * (8 * cap))()
        n = H.lib().dm_prof_rows(rows, cap)
    finally:
        out = (ctypes.c_double * (4 * 44))()
        H.lib().dm_prof_end(out, 44)
    assert 0 < n < cap
    return [tuple(int(rows[8 * i + j]) for j in range(6)) for i in range(n)]


def _print_rows(title, rows):
    print(f'\n[{title}] {len(rows)} tile-kernel launches: kind M N K splits flags   (kind = tile * 4 + a_layout * 2 + b_layout, + 24 on the '
          f'LDS-DMA loop; flags 1 gathered A, 2 gathered B, 4 scatter epilogue)')
    for r in rows:
        k = r[0] % 24
        print(f'  {r[0]:3d} {r[1]:9d} {r[2]:6d} {r[3]:9d} {r[4]:4d} {r[5]:3d}   {TILES[k // 4]} {"LDS-DMA" if r[0] >= 24 else "register-staged"}')
    print(f'  distinct tiles: {sorted({TILES[(r[0] % 24) // 4] for r in rows})}')


def test_dispatch_reaches_every_kernel_class(hip):
    """The depth-48 stack at 2 500 frames must really take the gathered-A, gathered-B and scatter-epilogue kernels, split-K, and
    both main loops - classes, not particular tiles - and run layer 1 of the encoder and the image layer of the decoder in the
    direct kernels (conv_direct.hip), i.e. NOT as tile-kernel products.  The tables go to the log, for 131 frames too."""
    oconf, _, model = _model(48, 3)
    big = _profiled_rows(hip, model, 2500, _inputs(oconf, 2500))
    _print_rows('dispatch at 2500 frames, depth 48', big)
    small = _profiled_rows(hip, model, 131, _inputs(oconf, 131))
    _print_rows('dispatch at 131 frames, depth 48', small)
    tiled = [r for r in big if r[0] < 20 or r[0] >= 24]       # kinds 20..22 are the row-panel / whole-MLP kernels
    assert any(r[5] & 1 for r in tiled), 'no gathered-A product'
    assert any(r[5] & 2 for r in tiled), 'no gathered-B product'
    assert any(r[5] & 4 for r in tiled), 'no scatter-epilogue product'
    assert any(r[4] > 1 for r in tiled), 'no split-K product'
    assert any(r[0] < 20 for r in tiled), 'no product on the register-staged loop'
    assert any(r[0] >= 24 for r in tiled), 'no product on the LDS-DMA loop'
    # the direct kernels are not in this table: with them on, no tile-kernel product has the shapes they replace
    n = 2500
    replaced = {'encoder layer 1 forward': lambda r: r[1] == n * 961 and r[3] == 48,
                'encoder layer 1 weight gradient': lambda r: r[3] == n * 961,
                'decoder image layer forward': lambda r: r[1] in (n * 900, n * 1024) and r[2] in (4 * 3, 36 * 3),
                'decoder image layer data / weight gradient': lambda r: (r[1] == n * 900 and r[3] == 144) or r[3] == n * 900}
    for what, hit in replaced.items():
        assert not any(hit(r) for r in big), f'{what} ran as a tile-kernel product: the direct kernel was not taken'
    before = hip.lib().dm_dec_l4_bwd_direct_enable(-1)
    hip.lib().dm_dec_l4_bwd_direct_enable(0)
    try:
        off = _profiled_rows(hip, model, 2500, _inputs(oconf, 2500))
    finally:
        hip.lib().dm_dec_l4_bwd_direct_enable(before)
    assert any(replaced['decoder image layer data / weight gradient'](r) for r in off), \
        'with the image layer\'s direct backward off its two products must appear (else the absence above proves nothing)'
    print(f'  direct kernels: none of {sorted(replaced)} appears among the tile-kernel launches at {n} frames; with '
          f'dm_dec_l4_bwd_direct_enable(0) the image layer\'s two backward products do: '
          f'{[r for r in off if replaced["decoder image layer data / weight gradient"](r)]}')


@pytest.mark.parametrize('bf16', [False, True], ids=['f32', 'bf16'])
def test_each_call_on_exactly_its_own_workspace_part(hip, bf16):
    """dm_workspace_query: the encoder backward, the decoder forward and the decoder backward each run on a canary-fenced
    workspace of exactly their own part and give the bits they give on dm_workspace_bytes; one 256-byte granule less is refused
    with DM_E_WORKSPACE before anything is launched (every output still holds its fill pattern).  cnn_depth 8, 3 frames."""
    oconf, _, model = _model(8, 3)
    frames, flags = 3, hip.DM_FLAG_BF16 if bf16 else 0
    inp = _inputs(oconf, frames)
    shp = _shape(model, frames, flags=flags)
    q = (ctypes.c_size_t * 8)()
    hip.call('dm_workspace_query', ctypes.byref(shp), q, 8)
    enc_bwd, dec_fwd, dec_bwd = int(q[1]), int(q[2]), int(q[3])
    print(f'parts (floats): encoder backward {enc_bwd}, decoder forward {dec_fwd}, decoder backward {dec_bwd}; '
          f'dm_workspace_bytes {hip.workspace_bytes(shp)}')
    assert min(enc_bwd, dec_fwd, dec_bwd) >= 16 * 1024 * 1024 and 4 * max(q) < hip.workspace_bytes(shp)
    full = {**{'enc ' + k: v for k, v in _run_encoder(hip, model, frames, inp, flags=flags).items()},
            **{'dec ' + k: v for k, v in _run_decoder(hip, model, frames, inp, flags=flags).items()}}
    own = {**{'enc ' + k: v for k, v in _run_encoder(hip, model, frames, inp, flags=flags, bwd_floats=enc_bwd).items()},
           **{'dec ' + k: v for k, v in _run_decoder(hip, model, frames, inp, flags=flags, fwd_floats=dec_fwd,
                                                     bwd_floats=dec_bwd).items()}}
    differ = [k for k in full if not torch.equal(full[k].view(torch.int32), own[k].view(torch.int32))]
    assert not differ, f'{differ} differ between a workspace of the call\'s own part and dm_workspace_bytes'
    assert all(bool(torch.isfinite(v).all()) for v in own.values())

    def refused(run, untouched, **kw):
        book = []
        with pytest.raises(hip.DreamerHipError, match='code -2.*workspace too small'):
            run(hip, model, frames, inp, flags=flags, book=book, **kw)
        torch.cuda.synchronize()
        checked = [b for b in book if b.name.startswith(untouched)]
        assert checked and all(bool((b.raw == CANARY).all()) for b in checked), f'{kw}: something was launched'

    refused(_run_encoder, 'encoder d', bwd_floats=enc_bwd, bwd_cut=256)
    refused(_run_decoder, ('decoder acts', 'loss_image', 'image_rec'), fwd_floats=dec_fwd, fwd_cut=256)
    refused(_run_decoder, 'decoder d', bwd_floats=dec_bwd, bwd_cut=256)
