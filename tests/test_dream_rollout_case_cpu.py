"""No GPU: the preconditions test_gpu_dream_rollout.py relies on, for every case of tests/dream_rollout_case.py's table.  A
changed oracle, generator layout or seed cannot silently turn a GPU case vacuous, and a case's hand-written schedule bits cannot
drift from the predicates of RolloutCtx::plan (csrc/rssm.hip) as dream_rollout_case.plan_bits restates them."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dream_rollout_case as RC                      # noqa: E402

ORACLE_CASES = [n for n, c in RC.CASES.items() if not c['bf16']]      # (the bf16 pairs are compared run against run)


@pytest.mark.parametrize('name', ORACLE_CASES)
def test_draws_stay_clear_of_the_cdf_edges(name):
    """Up to 301 rows: no draw of the case within EDGE of an fp64 CDF edge (the GPU test then demands ALL indices equal).  The
    16384-row case: at most 0.1 % of the rows inside it (they are left out there).  Every sampled quantity is finite and every
    row that draws at all has a finite distance."""
    case = RC.CASES[name]
    c = RC.case_inputs(case)
    ora = RC.oracle_run(c)
    good = RC.clear_rows(c, ora)                      # asserts the precondition
    assert torch.isfinite(ora['feat']).all() and torch.isfinite(ora['actions']).all()
    draws = c['kind'] == 0 or c['C'] != 0
    assert bool(torch.isfinite(ora['row_dist']).all()) == draws
    assert int(good.sum()) >= case['M'] - case['M'] // 1000
    if case['start'] == 'mixed':                      # the three kinds of start row are all there
        z0, r = c['z0'], torch.arange(c['M']) % 3
        assert bool((z0[r == 2] == 0).all()) and bool((c['h0'][r == 2] == 0).all())
        nz = (z0[r == 1] != 0).sum(-1)
        assert int(nz.min()) > c['S'] and int((z0[r == 1] == 0).sum(-1).min()) > 0      # dense, with exact zeros
        assert bool(((z0[r == 0] != 0).sum(-1) == c['S']).all())


@pytest.mark.parametrize('name', list(RC.CASES))
def test_case_bits_follow_the_plan_predicates(name):
    case = RC.CASES[name]
    want = RC.plan_bits(RC.conf_of(case['kw']), case['M'], case['H'], bf16=case['bf16'])
    assert case['bits'] == want, (name, RC.fmt(case['bits']), RC.fmt(want))


def test_every_schedule_bit_is_asserted_on_and_off():
    for k in RC.BITS:
        seen = {c['bits'][k] for c in RC.CASES.values()}
        assert seen == {True, False}, (k, seen)


def test_workspace_cuts_land_between_the_blocks():
    """plan_floats() against dm_workspace_bytes' own sizing needs the library; what holds without it: the cuts are ordered, a
    granule apart from the block they stop short of, and at the tiny width nothing that follows the z_mlp^T block fits into it
    (so that cut reports every bit off)."""
    c = RC.case_inputs(RC.CASES['ws-M300'])
    f = RC.plan_floats(c)
    cuts = [RC.cut_bytes(c, k) for k in ('must', 'wzt', 'wpack', 'add0')]
    assert cuts == sorted(cuts) and all(b % 256 == 0 for b in cuts)
    assert cuts[0] == 4 * (f['must'] - 64) and cuts[3] == 4 * (f['must'] + f['wzt'] + f['wpack'] + f['add0'] - 64)
    assert f['wpack'] > f['wzt'] and f['add0'] > f['wzt']
    assert f['wpack'] == 25 * 512 * (4 + 3 * 13)      # F = 128: 4 k-panels; 400: 13
    # the bits test_gpu_dream_rollout.py::test_workspace_fallbacks expects per cut
    oconf = c['oconf']
    assert RC.plan_bits(oconf, 300, 5, fits=('wzt', 'wpack')) == RC.bits('wzt+wat+actor_wpack+fuse_act')
    assert RC.plan_bits(oconf, 300, 5, fits=('wzt',)) == RC.bits('wzt+wat')
    assert RC.plan_bits(oconf, 300, 5, fits=()) == RC.bits('')


def test_fp32_oracle_is_within_the_feature_bar():
    """The bars are the project's own for these quantities; the same restatement in fp32 stays inside them against fp64 at the
    tiny width (were it not so, a bar would have to be derived from this floor, four times it)."""
    c = RC.case_inputs(RC.CASES['tiny-M37'])
    a, b = RC.oracle_run(c), RC.oracle_run(c, dtype=torch.float32)
    assert torch.equal(a['act_idx'], b['act_idx']) and torch.equal(a['lat_idx'], b['lat_idx'])
    assert RC.excess(b['feat'], a['feat']) <= 2e-5 / 4
