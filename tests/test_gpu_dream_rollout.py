"""-m gpu: dm_dream_rollout (csrc/rssm.hip RolloutCtx) at every branch of its launch schedule against the fp64 oracle.

The rollout picks its schedule from the shape, the precision flag and the workspace size alone.  Every case below drives it
stand-alone through the C-ABI (tests/dream_rollout_case.py), prints dm_rssm_last_schedule(2) and asserts its bits BEFORE any
value is compared, so none can pass on a path other than the one it names.  The expected bits are written out per case in
dream_rollout_case.CASES, from the predicates of RolloutCtx::plan; test_dream_rollout_case_cpu.py holds them against a
restatement of those predicates and checks every case's precondition without a GPU.

Bars, against fp64: features 2e-5 absolute (Gaussian z columns among them), kept actor outputs 2e-5 + 1e-5 relative, continuous
actions 1e-4 relative + 1e-5.  Draws: rows are independent in the rollout, so a flipped draw spoils its own row only.  Up to 301
rows: precondition - no draw of the case within EDGE = 1e-6 of an fp64 CDF edge - then ALL action and latent indices equal the
fp64 draw.  The 16384-row case: rows inside EDGE are left out (3 of 16384; at most 0.1 % asserted), all others are held to the
same bars.  No bar had to be derived from the fp32 oracle.

All cases: tiny width (deter 64, hidden 64, stoch 8x8, action_dim 6, heads 400 wide), H = 5, unless stated; MID = deter 256 /
hidden 256 / stoch 8x32.  ALL5 = wzt+wat+actor_wpack+actor_add0+fuse_act.  Seed = the first of 5, 6, ... with minimum distance >= 2e-6.

case                         expected bits                   read from                                         seed  min edge distance
tiny-M1 .. tiny-M255         wzt+wat                         dm_mlp_chain_ok: rows >= 256                      5     2.0e-5 7.5e-6 (M 65) .. 3.1e-6 (M 255)
tiny-M256, tiny-M301         ALL5                            dm_mlp_chain_ok, _sparse_ok, dm_z_embed_ok        5, 6  6.8e-6, 2.7e-6
mid-M1 .. mid-M255           wzt+wat                         as tiny                                           5     5.1e-4 3.4e-6 2.0e-6 2.8e-6 2.4e-6
mid-M256, mid-M301           ALL5                            as tiny                                           5, 9  2.4e-6, 2.5e-6
tiny-M16384-panel (H 2)      wzt+wat                         dm_panel_ok: rows >= 16384 at hidden 400          5     3 rows left out; others >= 1.3e-6
h1-M37 / -M300               none / actor_wpack+fuse_act     plan: H > 1 for wzt; add0 needs pidx              5     3.1e-4 / 1.6e-5
hd1028-M65 / -M300           none / actor_wpack+fuse_act     dm_z_embed_ok(Hd): n <= 1024                      5, 8  2.1e-5 / 6.2e-6
{tanh_normal,normal_tanh}-mid-M37, -M65   wzt                plan: wat for adist == 0 only                     5     5.9e-6 4.2e-6 / 3.3e-5 7.1e-6
{..}-M300 (action_dim 4)     wzt+actor_wpack+actor_add0      plan: fuse_act for adist == 0 only                5     6.9e-6 / 4.2e-6
{..}-A17-M300                wzt                             dm_mlp_chain_ok: out_dim 34 > 32                  5     2.6e-6 / 6.7e-6
A33-M300                     wzt+wat                         dm_mlp_chain_ok: out_dim 33 > 32                  5     3.7e-6
deter36-M300                 wzt+wat+actor_wpack+fuse_act    dm_mlp_chain_sparse_ok: dense % 8                 5     3.9e-6
gauss-M37 / -M300            none / actor_wpack+fuse_act     plan: C != 0 for wzt and add0                     5     5.8e-4 / 3.1e-5
gauss-tanh_normal-M37 / -M300  none / actor_wpack            no discrete draw at all                           5     -
gru_layernorm[_dv2]-M37      wzt+wat                         (the cell changes no bit but tw_on)               5     2.3e-5 / 2.9e-5
gru_layernorm[_dv2]-M300     ALL5                                                                              5     1.3e-5 / 8.8e-6
gru_layernorm[_dv2]-mid-M300 ALL5                                                                              12, 8 3.4e-6 / 2.5e-6
gru2-M37 / -M300             wzt+wat / ALL5                  gru_layers 2, deter 64                            5     3.5e-5 / 7.9e-6
gru4-deter96-M65 / -M300     wzt+wat / ALL5                  gru_layers 4, deter 96                            5     3.3e-5 / 5.4e-6
dv2x2-M65 / -M300            wzt+wat / ALL5                  gru_layernorm_dv2, 2 layers                       5     6.6e-6 / 1.1e-5
nonorm-M37 / -M300           wzt+wat                         dm_mlp_chain_ok: LayerNorm parameters             5     2.8e-6 / 5.9e-5
stoch5x12-M300               ALL5                            Z = 60, F = 124                                   5     4.9e-6
stoch40x32-M64 / -M300       wzt+wat / ALL5                  F = 1344 <= 4096                                  15, 267  2.9e-6 / 2.2e-6
stoch65x4-M64 / -M300        wzt+wat / ALL5                  F = 324                                           5, 12 1.2e-5 / 3.8e-6
mixed-start-M300             ALL5                            (step 0: dm_sparse_rows_launch on a dense z)      6     6.0e-6
keep-M65 / -M300             wzt+wat / ALL5                  (options change no bit)                           5     7.5e-6 / 1.6e-5
keep-tanh_normal-M300        wzt+actor_wpack+actor_add0                                                        5     6.9e-6
ws-M300                      ALL5, and per cut below         plan: the take-or-restore sites                   5     1.6e-5
twins-M64-H42 / -H39         wzt+wat+tw_on                   plan: tw_on; bf16 refuses dm_mlp_chain_sparse_ok  5     run against run
twins-M520-H42 / -H39        wzt+wat+actor_wpack+fuse_act+tw_on                                                5     run against run
"""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dream_rollout_case as RC                      # noqa: E402

pytestmark = pytest.mark.gpu

SPECIAL = ('keep-', 'ws-', 'twins-')
PLAIN = [n for n in RC.CASES if not n.startswith(SPECIAL)]


@functools.lru_cache(maxsize=None)
def _inputs_and_oracle(name):
    """(inputs, fp64 oracle) of a case: computed once, shared by the tests that need it, never modified."""
    c = RC.case_inputs(RC.CASES[name])
    return c, RC.oracle_run(c)


def _run(name, bits=None, **opts):
    c, ora = _inputs_and_oracle(name)
    RC.clear_rows(c, ora)                             # the precondition, before any GPU time is spent
    out = RC.run_case(c, RC.CASES[name]['bits'] if bits is None else RC.bits(bits), label=name, **opts)
    return c, ora, out


@pytest.mark.parametrize('name', PLAIN)
def test_rollout_vs_fp64(hip, name):
    """Sections 1 - 11 of the table: the schedule asserted, then every index equal to the fp64 draw and every value inside its
    bar.  What each case is pinned to:
    tiny / mid -M*: 1 row, the 64 / 65 edge of the <= 64-row products, 255 / 256 - the whole-MLP actor's floor -, 301 (a row count
    >= 256 that is no multiple of 4: the last workgroup of the one-wave-per-row gathers is ragged); 16384 rows: the row-panel
    actor.  h1: no gather at all.  hd1028: the z_mlp / a_mlp products and the LayerNorm launch at every step.  Continuous
    actors: the `add = ea` form of z_embed_kernel (a_mlp stays a product), the (H, M, A) noise, a 2A-wide actor output on the
    whole-MLP kernel.  A33 / A17: the plain GEMM + LayerNorm actor at >= 256 rows, with the one-hot draw behind it.  deter36: the
    whole-MLP kernel's dense first layer over all of [h | z].  gauss: no gather, no draw of z.  Cells: the LayerNorm GRUs and the
    stacks.  nonorm: the gather's activation-only form, the plain actor.  stoch5x12: S below the 8-group trip; 40x32: five trips;
    65x4: a second 64-index fetch and a tail of one.  mixed-start: step 0's first actor layer from a dense z, a one-hot z and
    the zero rows of init_state in one launch (the ballot scan of dm_sparse_rows_launch)."""
    c, ora, out = _run(name)
    RC.check(c, ora, out, name)
    assert torch.equal(out['feat'][0], torch.cat((c['h0'], c['z0']), -1)), 'feature rows of step 0 are the start state'


@pytest.mark.parametrize('name', ['keep-M65', 'keep-M300', 'keep-tanh_normal-M300'])
def test_kept_activations_change_no_value(hip, name):
    """actor_acts / actor_logits given (the trainer's call): features, actions and indices BIT-identical to the call without
    them, and each step's actor output - step i at row offset i * M of the (H * M)-row buffer - within 2e-5 + 1e-5 relative of
    the oracle's."""
    c, ora, plain = _run(name)
    _, _, kept = _run(name, keep_acts=True)
    for k in ('feat', 'actions', 'act_idx'):
        assert torch.equal(plain[k], kept[k]), (name, k)
    assert plain['logits'] is None and kept['logits'] is not None
    RC.check(c, ora, kept, name + ' kept')


@pytest.mark.parametrize('name', ['keep-M65', 'keep-M300', 'keep-tanh_normal-M300'])
def test_without_the_index_buffer(hip, name):
    """act_idx == NULL: the rollout's own `aidx` scratch feeds the a_mlp^T gather (one-hot actors); same schedule, features and
    actions BIT-identical to the call with the buffer."""
    c, ora, plain = _run(name)
    _, _, bare = _run(name, with_act_idx=False)
    assert bare['act_idx'] is None
    for k in ('feat', 'actions'):
        assert torch.equal(plain[k], bare[k]), (name, k)
    RC.check(c, ora, bare, name + ' act_idx=NULL')


def test_action_draw_as_its_own_launch(hip):
    """dm_rollout_fuse_act_enable(0): fuse_act off with the whole-MLP actor still on - the stand-alone sampler behind it."""
    c, ora, out = _run('keep-M300', bits='wzt+wat+actor_wpack+actor_add0', fuse_act=0)
    RC.check(c, ora, out, 'keep-M300 fuse_act=0')


@pytest.mark.parametrize('short_of,want', [('add0', 'wzt+wat+actor_wpack+fuse_act'), ('wpack', 'wzt+wat'), ('wzt', '')])
def test_workspace_fallbacks(hip, short_of, want):
    """A workspace that ends one 64-float granule short of an optional block of RolloutCtx::plan (dream_rollout_case.plan_floats
    restates the carving).  The reported bits prove the cut landed where intended, then all bars apply.
    add0: the actor's W0^T / addend block is refused and the mark restored - the whole-MLP kernel multiplies all of [h | z].
    wpack: the fragment-major actor weights are refused; with them goes add0 (taken only behind them) and the fused draw.  The
    actor still qualifies for the whole-MLP kernel, which then packs its weights into the split-K scratch at every step.
    wzt: the z_mlp^T / a_mlp^T / index block (7 232 floats at this shape) is refused and the mark restored; as read from the code
    NOTHING that follows fits into the room it leaves: the packed weights need 550 400 floats, and add0 is not tried without
    them and without pidx - every bit off."""
    c, ora = _inputs_and_oracle('ws-M300')
    out = RC.run_case(c, RC.bits(want), ws_bytes=RC.cut_bytes(c, short_of), label=f'ws-M300 short of {short_of}')
    RC.check(c, ora, out, f'ws-M300 short of {short_of}')


def test_workspace_of_exactly_the_rollout_part(hip):
    """dm_workspace_query's rollout part as the whole workspace: every optional block of RolloutCtx::plan still fits - the case's
    own bits - and all bars apply."""
    import ctypes
    c, ora = _inputs_and_oracle('ws-M300')
    shp = RC._model(c, False).wm.shape(1, c['M'], c['H'])
    parts = (ctypes.c_size_t * 8)()
    hip.call('dm_workspace_query', ctypes.byref(shp), parts, 8)
    fl = RC.plan_floats(c)
    assert int(parts[6]) == fl['must'] + fl['wzt'] + fl['wpack'] + fl['add0'] and 4 * int(parts[6]) < hip.workspace_bytes(shp)
    out = RC.run_case(c, RC.CASES['ws-M300']['bits'], ws_bytes=4 * int(parts[6]), label='ws-M300 on exactly the rollout part')
    RC.check(c, ora, out, 'ws-M300 on exactly the rollout part')


def test_workspace_short_of_the_mandatory_part(hip):
    """One granule short of what plan() must have: the workspace error, and nothing launched (every output still at its fill
    value after a device synchronise); one granule more and the call runs, with every optional block refused."""
    c, ora = _inputs_and_oracle('ws-M300')
    with pytest.raises(RC.RolloutRefused) as e:
        RC.run_case(c, RC.bits(''), ws_bytes=RC.cut_bytes(c, 'must'), label='ws-M300 short of must')
    assert 'workspace too small' in e.value.message, e.value.message
    assert e.value.untouched, 'the refused call wrote to its outputs'
    out = RC.run_case(c, RC.bits(''), ws_bytes=RC.cut_bytes(c, 'must') + 256, label='ws-M300 exactly must')
    RC.check(c, ora, out, 'ws-M300 exactly must')


@pytest.mark.parametrize('name', ['twins-M64-H42', 'twins-M64-H39', 'twins-M520-H42', 'twins-M520-H39'])
def test_bf16_twins_past_the_40_step_cap(hip, name):
    """DM_FLAG_BF16 at deter 400 / hidden 400 / stoch 8x8 (F = 464): K = 400 = DM_HSTORE_MIN_K_DENSE is the shortest reduction at
    which dm_gemm_launch reads twins for a dense product.  The twin map holds the h columns of steps 1 .. 39 only (`i < 40`): at
    H = 42 the last steps' products read fp32 storage, at H = 39 every step is twinned, so a failure of H = 42 alone points at
    the cap.  Twins on against twins off (same bf16 operand values, fp32 summation order differs), as
    test_dream_rollout_bf16_storage_twins_match_fp32_storage: a row is alive while all its draws so far are equal in both runs;
    at every step the h columns of alive rows agree within 2e-5, everything is finite, and at least half of the rows are alive
    at the end (the existing 5-step test's 90 % bounds flips at 6e-4 per draw: >= 80 % over 42 x 9 draws).
    64 rows (the issue's case): the three products with N K >= 64 K run on the skinny kernel, which keeps fp32 operands - only the
    prior's (64 x 400) product reads twins there.  520 rows: past the skinny kernel's 512, all four products read twins, the h
    columns of `feats` among them, which is what the cap is about; the whole-MLP actor runs in bf16 without its gathered layer.
    Alive at the end, as measured (printed as ALIVE): 100 % in all four cases, the h columns bit-identical throughout - with the
    same operand values the bf16-storage and the fp32-storage kernels also sum in the same order at these shapes."""
    case = RC.CASES[name]
    c = RC.case_inputs(case)
    on = RC.run_case(c, case['bits'], bf16=True, twins=1, label=name + ' twins=1')
    off = RC.run_case(c, dict(case['bits'], tw_on=False), bf16=True, twins=0, label=name + ' twins=0')
    D_, Hh = c['D'], c['H']
    for o in (on, off):
        assert torch.isfinite(o['feat']).all() and torch.isfinite(o['actions']).all()
    alive = torch.ones(c['M'], dtype=torch.bool)
    worst = 0.0
    for i in range(Hh):
        alive &= (on['act_idx'][i] == off['act_idx'][i]) & (on['feat'][i + 1, :, D_:] == off['feat'][i + 1, :, D_:]).all(-1)
        err = RC.excess(on['feat'][i + 1, alive, :D_], off['feat'][i + 1, alive, :D_])
        worst = max(worst, err)
        assert err <= 2e-5, (name, 'h of alive rows at step', i, err)
    share = float(alive.float().mean())
    print(f'ALIVE {name} share={share:.4f} worst_h={worst:.2e}')
    assert share >= 0.5, (name, share)
