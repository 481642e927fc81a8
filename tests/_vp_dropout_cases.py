"""The case table of the dropout-ON gradient checks of the viewport-prediction engine, shared by the host test (the reference
alone: tests/test_host_vp_dropout_oracle.py) and the GPU test (tests/test_gpu_vp_dropout_grads.py), with the one recipe both
build their weights, batch, MTIO permutations and float64 answer from.

The weights and data of every case are chosen by tie margin (the precedent: the trajectory-seed comment in
tests/test_gpu_bf16_modes.py, test_vp_gradients_on_the_split_dw_path): the host test proves that the oracle in float32 stays
inside the strict band of its own float64 run with ZERO elements outside, i.e. no ReLU gate or MaxPool route sits on a near-tie
that two correct fp32 implementations would decide differently.  Combinations that do NOT satisfy it and must not be used:
(77,10,10,512,bias) rep (164 elements of one linear1.weight), (256,3,4,512,bias) mix (a route flip, downConv.weight off by 4 %
of its maximum), (256,2,4,512,bias) mix.  Change a seed -> rerun the host test.

That check is necessary, not sufficient: the float32 oracle is ONE fp32 implementation, and a decision it happens to take like float64
can still sit inside fp32 rounding.  With the recipe seed, (4,5,15,512,bias) p_pe 0.2 / p_drop 0 has a ReLU pre-activation of 1.2e-7 in
the second decoder layer (step 8) where float32 deviates from float64 by up to 4.5e-6: the float32 oracle stayed inside the band
(0.0055 of it) and the engine, deciding that one gate the other way, left it by 27 widths in exactly that layer's linear1.weight.  So
the host test also asserts the TIE MARGIN of every case judged by the strict band (tie_margins below): each ReLU pre-activation, each
MaxPool top-two gap and each periodic-error branch point is further from zero, in float64, than the largest float32-against-float64
deviation found anywhere in its tensor.  Four cases missed that with the recipe's trajectory seed B * 7 + T and take the first seed
B * 7 + T + 1000 k that meets it (tseed below): (33,2,16,64) 0.38 -> 3.5, (130,7,3,128) 0.59 -> 1.1, (6,3,12,256) 0.77 -> 8.3,
(4,5,15,512) p_pe 0.2 / p_drop 0: 0.03 -> 2.9 (margin / deviation, the smaller branch).  The shapes judged by the relaxed criterion
have 10^6 gates and always some inside rounding -- that is what the criterion is for.
"""
import collections

import numpy as np
import torch

from oracle import vp_oracle as vo

SEED = 4242                     # dropout seed of every case
P_PE, P_DROP = 0.2, 0.1         # the engine's defaults (positional-encoding dropout, nn.Transformer's own)

Case = collections.namedtuple('Case', 'B S T d bias two_stream p_pe p_drop branches wseed tseed')


def _c(B, S, T, d, bias, two_stream=False, p_pe=P_PE, p_drop=P_DROP, branches=('rep', 'mix'), wseed=None, tseed=None):
    # weights make_state_dict(d, 40 + B + S, bias), data synthetic_trajectories(B, S, T, seed=B * 7 + T) unless a case names its own
    return Case(B, S, T, d, bias, two_stream, p_pe, p_drop, branches, 40 + B + S if wseed is None else wseed, B * 7 + T if tseed is None else tseed)


# (B, S, T, d, bias) -> the backward path the shape pins (csrc/vp_engine.hip dec_bwd_step / backward, csrc/dec_step.hip, csrc/norm.hip,
# csrc/attn.hip mansy_attn_deferred_kv_ok -- vec4_layout_ok needs dh == 64, so dh = 8 / 16 / 32 take the per-step accumulating form)
CASES = [
    # d = 64: unfused predictor / embed backward, atomic LayerNorm backward, per-step accumulating attention backward; T = 16 = LMAX; S = 2 -> M = 1
    _c(5, 5, 15, 64, True), _c(3, 16, 16, 64, False), _c(33, 2, 16, 64, True, tseed=1247),
    # S = T = 1: no next step (has_next false), emb_next null, one memory row
    _c(3, 1, 1, 64, False), _c(5, 1, 1, 512, True),
    # a single trajectory (a permutation of one row is the replicate branch)
    _c(1, 10, 10, 64, True, branches=('rep',)),
    # dh = 16, rows not a multiple of any block
    _c(130, 7, 3, 128, True, tseed=1913),
    # d = 256 (dh = 32): fused dec_tail_fwd / dec_head_bwd (edrop, drop3), LayerNorm partial slots, NON-deferred attention backward
    _c(7, 10, 10, 256, True), _c(6, 3, 12, 256, False, tseed=1054), _c(9, 4, 1, 256, True),
    # d = 512 (dh = 64): fused head, deferred cross K/V (attn_bwd_dq + attn_kvgrad), self-attention pull form
    _c(4, 5, 15, 512, True), _c(3, 16, 16, 512, False), _c(6, 3, 12, 512, True),
    # the real width: ragged 16-row groups of dec_head_bwd, dW over 760 rows (K % 32 != 0); relaxed criterion (B * d >= 40 * 512)
    _c(76, 10, 10, 512, True),
    # two half-batches: the mask index bases b0*d, b0*H*(i+1), b0*H*M of the second half, second LayerNorm slot set, side-stream dW
    _c(256, 3, 4, 512, False, two_stream=True), _c(256, 4, 3, 256, False, two_stream=True),
    # one probability at a time: dr() degenerates to no-drop per family
    _c(4, 5, 15, 512, True, p_pe=0.0, p_drop=0.1), _c(4, 5, 15, 512, True, p_pe=0.2, p_drop=0.0, tseed=1043),
]

# the fused step (mansy_vp_train_step) is checked at one case per width
FUSED_CASES = [CASES[0], CASES[7], CASES[10]]
assert [c.d for c in FUSED_CASES] == [64, 256, 512]


# the split-bf16 modes: the setting of test_vp_gradients_on_the_split_dw_path (tests/test_gpu_bf16_modes.py) -- B = 32 makes every reduce
# dimension a multiple of the 32-k tile; weights 21, trajectory seed 5
SPLIT_BF16_CASE = _c(32, 10, 10, 64, True, branches=('rep',), wseed=21, tseed=5)


def case_id(c):
    s = f'B{c.B}_S{c.S}_T{c.T}_d{c.d}_{"bias" if c.bias else "nobias"}'
    if c.two_stream:
        s += '_2s'
    if (c.p_pe, c.p_drop) != (P_PE, P_DROP):
        s += f'_pe{c.p_pe:g}_drop{c.p_drop:g}'
    return s


def case_branches(cases=None):
    return [(c, b) for c in (CASES if cases is None else cases) for b in c.branches]


def cb_id(cb):
    return case_id(cb[0]) + '-' + cb[1]


def relaxed(c):
    """From B * d >= 40 * 512 up a near-tie flip moves single gradient elements (tests/test_gpu_vp_engine.py, edge shapes)."""
    return c.B * c.d >= 40 * 512


def mix_seed(c):
    return c.B + c.T


def mix_perms(c):
    """The two row permutations of the mix branch: what np.random.seed(mix_seed) followed by two np.random.shuffle(arange(B))
    (ViewportTransformerMTIO._mix_decision's order) draws."""
    rs = np.random.RandomState(mix_seed(c))
    return [rs.permutation(c.B) for _ in range(2)]


def inputs(c, branch):
    """-> (sd, (history, current, future), (src, cur, gt)): weights, raw batch and its MTIO mix, all float32 on the host."""
    sd = vo.make_state_dict(c.d, c.wseed, bias=c.bias)
    h, cu, f = vo.synthetic_trajectories(c.B, c.S, c.T, seed=c.tseed)
    perms = None if branch == 'rep' else [torch.from_numpy(p) for p in mix_perms(c)]
    return sd, (h, cu, f), vo.mtio_mix(h, cu, f, 3, branch == 'rep', perms)


_ANSWERS = {}


def fp64_answer(c, branch):
    """pred, loss, every gradient and the BatchNorm running statistics of one dropout-ON train step in float64.  The cases more than one
    test asks for are computed once and shared (callers must not modify the answer); the others are not kept (75 MB each at d = 512)."""
    key = (c, branch)
    if key in _ANSWERS:
        return _ANSWERS[key]
    sd, _, (src, cur, gt) = inputs(c, branch)
    pred, loss, grads, bn = vo.grads_fp64(sd, src, cur, gt, c.T, SEED, c.p_pe, c.p_drop)
    out = dict(pred=pred, loss=loss, grads=grads, bn=bn, gt=gt)
    if c in FUSED_CASES or c == SPLIT_BF16_CASE:
        _ANSWERS[key] = out
    return out


def _decision_quantities(c, branch, dtype):
    """Every quantity whose SIGN decides where a gradient goes: the pre-activations of each linear1 (ReLU gate), the gap between the
    two largest values of each MaxPool window (arg-max route), |pred - gt| - 1/2 (which branch of the periodic error)."""
    sd, _, (src, cur, gt) = inputs(c, branch)
    full = {k: (v.to(dtype) if v.dtype.is_floating_point else v) for k, v in sd.items()}
    orc = vo.VPOracle(full, fut_window=c.T, p_pe=c.p_pe, p_drop=c.p_drop)
    with torch.no_grad():
        pred, im = orc.process_src_current(src.to(dtype), cur.to(dtype), train=True, dropout_seed=SEED, want_intermediates=True)
    q = {}
    for l in range(orc.E):
        p = f'transformer.encoder.layers.{l}.'
        q[f'enc{l}.relu'] = vo._lin(im[f'enc{l}.y1'], full, p + 'linear1.weight', p + 'linear1.bias')
    for l in range(orc.D):
        p = f'transformer.decoder.layers.{l}.'
        q[f'dec{l}.relu'] = vo._lin(im[f'dec{l}.y2'], full, p + 'linear1.weight', p + 'linear1.bias')
    y = im['dis.act']
    ninf = torch.full((c.B, 1, c.d), float('-inf'), dtype=dtype)
    yp = torch.cat([ninf, y, ninf], dim=1)
    gaps = []
    for m in range((c.S - 1) // 2 + 1):
        w = yp[:, 2 * m:2 * m + 3]
        if torch.isfinite(w).sum(1).min() >= 2:
            t = w.topk(2, dim=1).values
            gaps.append(t[:, 0] - t[:, 1])
    if gaps:
        q['maxpool'] = torch.stack(gaps)
    q['loss'] = (pred - gt.to(dtype)).abs() - 0.5
    return q


def tie_margins(c, branch):
    """{quantity: (smallest |value| in float64, largest float32-against-float64 deviation of the quantity)}, from the oracle alone.  A
    decision whose exact value is further from zero than the largest deviation fp32 arithmetic produced ANYWHERE in its tensor goes the
    same way in every fp32 implementation; one that is much closer is a coin toss, and ONE flipped gate carries ~1 / rows of a
    gradient's scale -- tens of band widths at these row counts."""
    q64, q32 = _decision_quantities(c, branch, torch.float64), _decision_quantities(c, branch, torch.float32)
    return {k: (v.abs().min().item(), (q32[k].double() - v).abs().max().item()) for k, v in q64.items()}


def band(ref):
    """The strict band of a gradient tensor (numpy, float64 reference)."""
    return 3e-4 * np.abs(ref).max() + 2e-6


def cap(ref):
    return 1e-2 * np.abs(ref).max() + 2e-6


def grad_report(got, ref64, relaxed):
    """got / ref64: {name: tensor}.  -> (bad, worst): `bad` lists the tensors that miss the criterion -- the strict band on every
    element, or with `relaxed` (the GPU test: from B * d >= 40 * 512 up) at most max(8, 0.5 %) of a tensor's elements outside the band and none beyond 1e-2 of its
    maximum; `worst` = (largest error-to-band ratio over all tensors, its tensor)."""
    bad, worst = [], (0.0, None)
    assert sorted(got) == sorted(ref64), (sorted(got), sorted(ref64))
    for k, ref in ref64.items():
        ref = ref.numpy()
        g = got[k].detach().cpu().double().numpy()
        assert g.shape == ref.shape, (k, g.shape, ref.shape)
        err = np.abs(g - ref)
        tol = band(ref)
        if not np.isfinite(err).all():
            bad.append((k, 'non-finite'))
            continue
        ratio = float(err.max() / tol)
        if ratio > worst[0]:
            worst = (ratio, k)
        n_out = int((err > tol).sum())
        if relaxed:
            ok = n_out <= max(8, 5e-3 * err.size) and err.max() <= cap(ref)
        else:
            ok = n_out == 0
        if not ok:
            bad.append((k, float(err.max()), float(tol), n_out))
    return bad, worst
