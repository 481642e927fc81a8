"""The reference ALONE, for the dropout-ON gradient checks of tests/test_gpu_vp_dropout_grads.py (no GPU):

  (a) the oracle in float32 against the oracle in float64, dropout on, at every case and MTIO branch of the shared table
      (tests/_vp_dropout_cases.py): every gradient element inside 3e-4 * max|ref| + 2e-6 -- the band of
      test_edge_shapes_forward_loss_grads_vs_oracle -- with ZERO elements outside, also at the shapes the GPU test judges by the
      relaxed criterion.  So the chosen weights and data carry no ReLU-gate / MaxPool-route near-tie that two correct fp32
      implementations would decide differently.  Necessary, not sufficient -- so also: the tie margin of every decision point
      (ReLU gates, MaxPool routes, periodic-error branches) of the strict cases exceeds the fp32 rounding of its tensor.  With
      both, a GPU miss at these cases is the engine's.
  (b) the GPU test can fail: one dropout site drawing ANOTHER mask (a wrong site / step index on the backward side), for one
      representative of every site family, moves some float64 gradient tensor by more than 1e-2 of its maximum -- 33 x the strict
      band and the cap of the relaxed criterion, so either criterion catches it.  Measured (in band widths): 372 .. 8749 at
      (5,5,15,64), 390 .. 5063 at (4,5,15,512).  One more mutation drops the 1 / (1 - p) scale at one site (547 / 884 band widths).
"""
import numpy as np
import pytest
import torch

import _vp_dropout_cases as dc
from oracle import vp_oracle as vo


@pytest.mark.parametrize('cb', dc.case_branches() + dc.case_branches([dc.SPLIT_BF16_CASE]), ids=dc.cb_id)
def test_fp32_oracle_inside_the_strict_band_of_its_fp64_run(cb):
    c, branch = cb
    sd, _, (src, cur, gt) = dc.inputs(c, branch)
    ref = dc.fp64_answer(c, branch)
    pred, loss, grads, bn = vo.grads_autograd(sd, src, cur, gt, c.T, dc.SEED, c.p_pe, c.p_drop, dtype=torch.float32)
    assert pred.dtype == torch.float32 and ref['pred'].dtype == torch.float64 and all(g.dtype == torch.float64 for g in ref['grads'].values())
    np.testing.assert_allclose(pred.numpy(), ref['pred'].numpy(), atol=1e-4, rtol=0)
    np.testing.assert_allclose(loss.item(), ref['loss'].item(), rtol=1e-4, atol=1e-7)
    for a, b in zip(bn, ref['bn']):
        np.testing.assert_allclose(a.numpy(), b.numpy(), atol=1e-6, rtol=1e-5)
    bad, worst = dc.grad_report(grads, ref['grads'], relaxed=False)          # zero elements outside the band at EVERY case
    print('fp32 oracle vs fp64 oracle %s: worst error / band %.4f (%s)' % (dc.cb_id(cb), worst[0], worst[1]))
    assert not bad, bad
    # dropout is really on: the answer differs from the dropout-off one
    if branch == 'rep' and c is dc.CASES[0]:
        off = vo.grads_fp64(sd, src, cur, gt, c.T, None, c.p_pe, c.p_drop)
        assert (off[0] - ref['pred']).abs().max().item() > 1e-3


@pytest.mark.parametrize('cb', dc.case_branches() + dc.case_branches([dc.SPLIT_BF16_CASE]), ids=dc.cb_id)
def test_no_decision_of_a_strict_case_sits_inside_fp32_rounding(cb):
    """(a) is necessary, not sufficient (see tests/_vp_dropout_cases.py): every ReLU gate, MaxPool route and periodic-error branch of a
    case judged by the strict band is further from its tie, in float64, than float32 deviates from float64 anywhere in that tensor.
    The relaxed shapes, and the split-bf16 case whose setting is the one of test_vp_gradients_on_the_split_dw_path, are reported only."""
    c, branch = cb
    tm = dc.tie_margins(c, branch)
    print('tie margins %s: ' % dc.cb_id(cb) + ', '.join('%s %.1e / %.1e' % (k, m, d) for k, (m, d) in tm.items()))
    if not dc.relaxed(c) and c != dc.SPLIT_BF16_CASE:
        close = {k: v for k, v in tm.items() if not v[0] >= v[1]}
        assert not close, close


def test_fp64_helper_leaves_the_fp32_path_as_the_existing_tests_build_it():
    """grads_autograd in float32 == the recipe of test_edge_shapes_forward_loss_grads_vs_oracle, bit for bit."""
    c = dc.CASES[0]
    sd, _, (src, cur, gt) = dc.inputs(c, 'rep')
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items()
              if v.dtype.is_floating_point and 'running_' not in k and k != 'positional_embedding.pe'}
    full = dict(sd)
    full.update(params)
    orc = vo.VPOracle(full, fut_window=c.T)
    loss = orc.loss_function(orc.process_src_current(src, cur, train=True, dropout_seed=dc.SEED), gt)
    loss.backward()
    _, l2, grads, _ = vo.grads_autograd(sd, src, cur, gt, c.T, dc.SEED, 0.2, 0.1, dtype=torch.float32)
    assert loss.item() == l2.item() and sorted(grads) == sorted(params)
    for k, p in params.items():
        assert torch.equal(p.grad, grads[k]), k


def test_mix_permutations_are_the_models_host_rng_draws():
    """mix_perms == np.random.seed(mix_seed) + two np.random.shuffle(arange(B)): what _mix_decision draws in the GPU test."""
    c = dc.CASES[6]
    np.random.seed(dc.mix_seed(c))
    for want in dc.mix_perms(c):
        idx = np.arange(c.B)
        np.random.shuffle(idx)
        np.testing.assert_array_equal(idx, want)


# ---------------------------------------------------------------- (b) sensitivity
SENS_CASES = [dc.CASES[0], dc.CASES[10]]
assert [(c.B, c.S, c.T, c.d) for c in SENS_CASES] == [(5, 5, 15, 64), (4, 5, 15, 512)]
N_DEC = 2
OTHER = 500000                    # added to a site number: a site nothing else uses


def _mutations(T):
    m = [('pe_src', 'SITE_PE_SRC', None)]
    m += [(f'enc0_k{k}', 'site_enc', (0, k)) for k in range(4)]
    m += [(f'pe_tgt{i}', 'site_pe_tgt', (i,)) for i in (0, T - 1)]
    m += [(f'dec{l}_i{i}_k{k}', 'site_dec', (l, i, k)) for (l, i) in ((0, 0), (N_DEC - 1, T - 1)) for k in range(6)]
    return m


def _moved(c, ref):
    """max over tensors of max|g_mutated - g| / (1e-2 * max|g|), float64 against float64."""
    sd, _, (src, cur, gt) = dc.inputs(c, 'rep')
    _, _, grads, _ = vo.grads_fp64(sd, src, cur, gt, c.T, dc.SEED, c.p_pe, c.p_drop)
    worst = (0.0, None)
    for k, r in ref['grads'].items():
        scale = r.abs().max().item()
        if scale < 1e-7:
            continue
        ratio = (grads[k] - r).abs().max().item() / (1e-2 * scale)
        if ratio > worst[0]:
            worst = (ratio, k)
    return worst


@pytest.mark.parametrize('c', SENS_CASES, ids=dc.case_id)
def test_one_site_drawing_another_mask_leaves_the_cap(c, monkeypatch):
    ref = dc.fp64_answer(c, 'rep')
    report = []
    for name, fn, args in _mutations(c.T):
        with monkeypatch.context() as mp:
            if args is None:
                mp.setattr(vo, fn, getattr(vo, fn) + OTHER)
            else:
                orig = getattr(vo, fn)
                mp.setattr(vo, fn, lambda *a, _o=orig, _args=args: _o(*a) + (OTHER if a == _args else 0))
            ratio, k = _moved(c, ref)
        report.append((name, ratio, k))
    print('sensitivity %s, movement in band widths: ' % dc.case_id(c) + ', '.join('%s %.0f' % (n, r * 1e-2 / 3e-4) for n, r, _ in report))
    weak = [r for r in report if not r[1] > 1.0]
    assert not weak, weak
    assert vo.SITE_PE_SRC == 1 and vo.site_dec(1, 2, 3) == 10000 + (64 + 2) * 8 + 3        # the patches are gone


@pytest.mark.parametrize('c', SENS_CASES, ids=dc.case_id)
def test_one_site_without_its_scale_leaves_the_cap(c, monkeypatch):
    """A missing 1 / (1 - p) at one site (the first decoder layer's dropout1 at step 0, p = 0.1)."""
    ref = dc.fp64_answer(c, 'rep')
    site = vo.site_dec(0, 0, 1)
    orig = vo.Dropper.__call__

    def unscaled(self, x, s, p):
        y = orig(self, x, s, p)
        return y * (1.0 - p) if s == site else y
    with monkeypatch.context() as mp:
        mp.setattr(vo.Dropper, '__call__', unscaled)
        ratio, k = _moved(c, ref)
    print('missing scale %s: movement %.0f band widths (%s)' % (dc.case_id(c), ratio * 1e-2 / 3e-4, k))
    assert ratio > 1.0, (ratio, k)
