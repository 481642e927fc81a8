"""GPU parity of the split-bf16 precision modes of the dense products (csrc/gemm_bf16s.hip; BASELINE.json configs[4] "bf16 MFMA"):
  * the product itself, every operand layout / epilogue / split-K form, against a float64 product;
  * the reference goldens of the viewport predictor (tests/golden/vp_*.npz) in both modes: outputs within 1e-4, tile
    decisions bit-equal; gradients at the fp32 tolerance in bf16x6 and at a stated looser one in bf16x3;
  * the reference goldens of the bitrate-selection nets (ppo_reference.npz): logits / values / identifier outputs within
    1e-4, argmax decisions identical, identifier training;
  * config C5: identifier training + the 8-preference table (4 train + 4 test vectors, config.yml:141-144) in one
    vectorised environment, a full collect -> train identifier -> relabel -> PPO update cycle per mode.
The measured errors per variant are written by tools/bf16_modes_report.py (profiles/r02_bf16_modes_parity.txt)."""
import glob
import os
import random

import numpy as np
import _golden
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ppo_oracle as po  # noqa: E402
from oracle import vp_oracle as vo  # noqa: E402

HERE = os.path.dirname(__file__)
GOLD = sorted(p for p in glob.glob(os.path.join(HERE, 'golden', 'vp_*.npz')) if 'vp_loop_' not in os.path.basename(p))
IDS = [os.path.basename(p)[:-4] for p in GOLD]
ZP = _golden.load(os.path.join(HERE, 'golden', 'ppo_reference.npz'))
MODES = ['bf16x3', 'bf16x6']
# max |C - C64| / max |C64| of one product on N(0,1) operands: fp32 accumulation ~1e-6; the bf16x3 variant drops the
# a1*b1, a0*b2, a2*b0 terms (~3 * 2^-16 per element product, random signs)
GEMM_TOL = {'f32': 4e-6, 'bf16x3': 2e-5, 'bf16x6': 4e-6}


@pytest.fixture(scope='module')
def K():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a ROCm device (no CPU fallback exists)')
    from mansy_immersivevideostreaming_amd import kernels
    yield kernels
    kernels.set_precision('f32')


@pytest.fixture(autouse=True)
def _restore_mode():
    yield
    if torch.cuda.is_available():
        from mansy_immersivevideostreaming_amd import kernels
        kernels.set_precision('f32')


def test_mode_switch_api(K):
    assert K.get_precision() == 'f32'
    assert K.set_precision('bf16x3') == 'f32' and K.get_precision() == 'bf16x3'
    with K.precision('bf16x6'):
        assert K.get_precision() == 'bf16x6'
        with K.precision(None):
            assert K.get_precision() == 'bf16x6'
    assert K.get_precision() == 'bf16x3'
    K.set_precision('f32')
    with pytest.raises(Exception):
        K.set_precision('fp8')
    # ABI 8: the mode is host-side state of the calling thread; the library has no setter and rejects codes it does not know per call
    from mansy_immersivevideostreaming_amd._lib import lib
    assert not hasattr(lib(), 'mansy_set_gemm_precision') and not hasattr(lib(), 'mansy_get_gemm_precision')
    A = torch.randn(64, 32).cuda()
    with pytest.raises(Exception):
        K.gemm(A, A, prec=5)
    with pytest.raises(Exception):
        K.gemm(A, A, prec=-1)
    assert K.get_precision() == 'f32'


SHAPES = [  # (M, N, K) -- ragged rows / columns, one-tile and many-tile cases, the VP and PPO shapes
    (64, 64, 32), (1, 4, 32), (130, 68, 64), (257, 516, 96), (4096, 512, 512), (300, 1536, 512), (256, 1280, 768), (512, 128, 1280),
    (1024, 1024, 2048),
]


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('akm,bkm', [(0, 0), (0, 1), (1, 1), (1, 0)])
def test_split_product_all_layouts(K, mode, akm, bkm):
    g = torch.Generator().manual_seed(3)
    for M, N, Kd in SHAPES:
        if (akm and M % 4) or (bkm and N % 4):
            continue                                   # unaligned K-major operands stay on the fp32 fallback loop
        A = torch.randn((Kd, M) if akm else (M, Kd), generator=g).cuda()
        B = torch.randn((Kd, N) if bkm else (N, Kd), generator=g).cuda()
        ref = (A.double().t() if akm else A.double()) @ (B.double() if bkm else B.double().t())
        for tile in (0, 64, 128):
            with K.precision(mode):
                C = K.gemm(A, B, bool(akm), bool(bkm), force_tile=tile)
            err = ((C.double() - ref).abs().max() / ref.abs().max()).item()
            assert err < GEMM_TOL[mode], (mode, akm, bkm, M, N, Kd, tile, err)


@pytest.mark.parametrize('mode', MODES)
def test_split_product_is_not_the_fp32_product_and_bf16x6_is_tighter(K, mode):
    """The mode really switches the arithmetic: the result differs from the exact-fp32 product in the low bits, and the
    6-product variant sits an order of magnitude closer to the float64 product than the 3-product one."""
    g = torch.Generator().manual_seed(11)
    A, B = torch.randn(512, 512, generator=g).cuda(), torch.randn(512, 512, generator=g).cuda()
    ref = A.double() @ B.double().t()
    C32 = K.gemm(A, B)
    with K.precision(mode):
        Cm = K.gemm(A, B)
    assert not torch.equal(C32, Cm)
    with K.precision('bf16x3'):
        e3 = (K.gemm(A, B).double() - ref).abs().max().item()
    with K.precision('bf16x6'):
        e6 = (K.gemm(A, B).double() - ref).abs().max().item()
    assert e6 * 3 < e3, (e3, e6)


@pytest.mark.parametrize('mode', MODES)
def test_split_product_epilogues_and_split_k(K, mode):
    g = torch.Generator().manual_seed(5)
    M, N, Kd = 384, 256, 512
    A, B = torch.randn(M, Kd, generator=g).cuda(), torch.randn(N, Kd, generator=g).cuda()
    bias, resid = torch.randn(N, generator=g).cuda(), torch.randn(M, N, generator=g).cuda()
    mask = (torch.rand(M, N, generator=g) > 0.3).float().cuda()
    ref = A.double() @ B.double().t()
    tol = GEMM_TOL[mode] * ref.abs().max().item()
    with K.precision(mode):
        C = K.gemm(A, B, bias=bias, relu=True, resid=resid)
        want = torch.relu(ref + bias.double()) + resid.double()
        assert (C.double() - want).abs().max().item() < tol
        C = K.gemm(A, B, mask_src=mask, mask_scale=1.25)
        assert (C.double() - ref * mask.double() * 1.25).abs().max().item() < 1.25 * tol
        # dropout epilogue: the same counter hash as the fp32 loop -> identical keep pattern
        Cd = K.gemm(A, B, drop=(0.25, 7, 3))
    C0 = K.gemm(A, B, drop=(0.25, 7, 3))
    assert torch.equal(Cd == 0, C0 == 0)
    # split-K with atomics (dW form: K-major operands, accumulate) and an odd forced split count
    At, Bt = torch.randn(4096, 256, generator=g).cuda(), torch.randn(4096, 192, generator=g).cuda()
    refw = At.double().t() @ Bt.double()
    for splits in (0, 3, 8):
        out = torch.full((256, 192), 0.5, device='cuda')
        with K.precision(mode):
            K.gemm(At, Bt, True, True, out=out, accumulate=True, force_splitk=splits)
        assert ((out.double() - 0.5 - refw).abs().max() / refw.abs().max()).item() < GEMM_TOL[mode], splits
    # K not a multiple of 32: stays on the exact fp32 loops in every mode (bit-identical to the fp32 mode)
    A2, B2 = torch.randn(100, 72, generator=g).cuda(), torch.randn(60, 72, generator=g).cuda()
    with K.precision(mode):
        Cx = K.gemm(A2, B2)
    assert torch.equal(Cx, K.gemm(A2, B2))


@pytest.mark.parametrize('mode', ['f32'] + MODES)
def test_bias_gradient_rider_counts_every_k_tile_once(K, mode):
    """a_rowsum (the bias gradient riding on a dW = dY^T X product: dY is the K-major A) against dY.sum(0), for 1, 2, 3 and many
    K-tiles per split, forced split counts, both tiles -- the two-stage split-bf16 loops re-stage the final tile in their last,
    branch-free iteration and once counted it twice (+1 / (K-tiles per split))."""
    g = torch.Generator().manual_seed(17)
    for Kd in (32, 64, 96, 320, 4096):
        for M, N in ((64, 64), (512, 192), (132, 516)):
            dY = (torch.randn(Kd, M, generator=g) + 0.5).cuda()       # non-zero mean: a double-counted tile shows
            X = torch.randn(Kd, N, generator=g).cuda()
            want_c = dY.double().t() @ X.double()
            want_r = dY.double().sum(0)
            for tile in (0, 64, 128):
                for splits in ((0, 1, 2, 5) if Kd >= 320 else (0, 1)):
                    out = torch.zeros(M, N, device='cuda')
                    rs = torch.full((M,), 0.25, device='cuda')
                    with K.precision(mode):
                        K.gemm(dY, X, True, True, out=out, accumulate=True, force_tile=tile, force_splitk=splits, a_rowsum=rs)
                    tag = (mode, Kd, M, N, tile, splits)
                    assert ((out.double() - want_c).abs().max() / want_c.abs().max()).item() < GEMM_TOL[mode], tag
                    err = ((rs.double() - 0.25 - want_r).abs().max() / want_r.abs().max()).item()
                    # (fp32 running sums over Kd terms; a double-counted 32-k tile would be 32 / Kd >= 8e-3)
                    assert err < (2e-6 if Kd <= 320 else 2e-5), tag + (err,)
    # per-product precision override (mansy_gemm_epilogue.prec) does what the process-wide mode does
    dY, X = torch.randn(256, 128, generator=g).cuda(), torch.randn(256, 128, generator=g).cuda()
    pm = {'f32': 0, 'bf16x3': 3, 'bf16x6': 6}[mode]
    with K.precision(mode):
        a = K.gemm(dY, X, True, True)
    assert torch.equal(a, K.gemm(dY, X, True, True, prec=pm)) and K.get_precision() == 'f32'


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('bias', [True, False])
def test_vp_gradients_on_the_split_dw_path(K, mode, bias):
    """Every dW / bias-gradient product of the engine on the split-bf16 loops: B = 32 makes every reduce dimension (320 encoder
    rows, 160 memory rows, T x 32 stacked decoder rows) a multiple of the 32-k tile -- the reference goldens have B = 4..8, where
    those products fall back to the exact fp32 loop.  Against the oracle's autograd on the same weights and batch."""
    from mansy_immersivevideostreaming_amd.viewport_prediction.models import mtio
    d, S, T, B = 64, 10, 10, 32
    sd = vo.make_state_dict(d, 21, bias=bias)
    m = mtio.ViewportTransformerMTIO(in_channel=2, fut_window=T, d_model=d, dim_feedforward=d, device='cuda', bias=bias)
    m.load_state_dict(sd)
    m = m.to('cuda')
    m.dropout_p = m.attn_dropout_p = 0.0
    m.repeat_prob = 1.0
    m.train()
    # (trajectory seed 5: the closest two values of any MaxPool window are 1.2e-4 / 3.2e-5 apart -- the arg-max routing of the
    # gradient is then the same in every fp32 implementation; see tools/gen_golden_vp_c1.py)
    h, c, f = vo.synthetic_trajectories(B, S, T, seed=5)
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items()
              if v.dtype.is_floating_point and 'running_' not in k and k != 'positional_embedding.pe'}
    full = dict(sd)
    full.update(params)
    orc = vo.VPOracle(full, fut_window=T)
    src, cur, gt = vo.mtio_mix(h, c, f, 3, True, None)
    oloss = orc.loss_function(orc.process_src_current(src, cur, train=True), gt)
    oloss.backward()
    got = {}
    for md in ('f32', mode):
        m.precision = None if md == 'f32' else md
        opt = mtio.FusedAdamW(m, lr=1e-4)
        opt.zero_grad()
        pred, g2 = m(h.cuda(), c.cuda(), f.cuda())
        loss = m.loss_function(pred, g2)
        loss.backward()
        assert abs(loss.item() - oloss.item()) < 1e-4 * abs(oloss.item())
        got[md] = {k: p.grad.detach().cpu().clone() for k, p in m.named_parameters()}
    assert K.get_precision() == 'f32'
    bad = []
    for k, p in params.items():
        ref = p.grad
        scale = ref.abs().max().item()
        if scale < 1e-7:           # parameters whose true gradient is zero (conv bias before the BatchNorm, key biases)
            continue
        e32 = (got['f32'][k] - ref).abs().max().item() / scale
        em = (got[mode][k] - ref).abs().max().item() / scale
        if e32 > 2e-4 or em > GRAD_TOL[mode]:
            bad.append((k, e32, em))
    print('BAD', bad)
    assert not bad, bad
    # the bias gradients specifically: a mis-counted K-tile is a relative error of 1/10 .. 1/1 on them
    for k in params:
        if k.endswith('bias') and params[k].grad.abs().max().item() > 1e-6:
            rel = (got[mode][k] - params[k].grad).norm().item() / params[k].grad.norm().item()
            assert rel < (2e-2 if mode == 'bf16x3' else 1e-3), (k, rel)


# ------------------------------------------------------------------ viewport predictor against the reference goldens
def _build_vp(z, mode):
    from mansy_immersivevideostreaming_amd.viewport_prediction.models import mtio
    sd = vo.make_state_dict(int(z['d']), int(z['wseed']), bias=bool(z['bias']))
    d = int(z['d'])
    m = mtio.ViewportTransformerMTIO(in_channel=2, fut_window=int(z['T']), d_model=d, dim_feedforward=d, device='cuda', bias=bool(z['bias']))
    m.load_state_dict(sd)
    m = m.to('cuda')
    m.dropout_p = 0.0
    m.attn_dropout_p = 0.0
    m.precision = mode
    return mtio, m


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('path', GOLD, ids=IDS)
def test_vp_eval_and_sample_vs_reference_golden(K, path, mode):
    z = _golden.load(path)
    _, m = _build_vp(z, mode)
    m.eval()
    h, c = torch.from_numpy(z['history']).cuda(), torch.from_numpy(z['current']).cuda()
    with torch.no_grad():
        pred = m._process_src_current(torch.cat([h] * 3, -1), torch.cat([c] * 3, -1))
        samp = m.sample(h, c)
    assert K.get_precision() == 'f32'                       # the model-level mode does not leak
    np.testing.assert_allclose(pred.cpu().numpy(), z['eval_pred'], atol=1e-4, rtol=0)
    np.testing.assert_allclose(samp.cpu().numpy(), z['eval_sample'], atol=1e-4, rtol=0)
    got = K.tilemap(samp).cpu().numpy().reshape(-1)
    want = K.tilemap(torch.from_numpy(z['eval_sample']).cuda()).cpu().numpy().reshape(-1)
    if mode == 'bf16x6':
        np.testing.assert_array_equal(got, want)            # tile-index decisions bit-exact (north_star), as in fp32
    else:
        # bf16x3 moves an output by up to ~1e-5 (pixel coordinate = int(x * 2560)): a point that close to a pixel that starts a new
        # tile column / row flips -- none on the synthetic goldens, 1 of 320 on the real-trace B = 32 batch (the C1 fixture).  The
        # asserted threshold: at most 1 tile-map decision in 256 differs from the reference's, and every
        # differing map must come from a point within 2e-5 of the reference's.
        diff = got != want
        assert diff.mean() <= 1.0 / 256, (diff.sum(), diff.size)
        err = np.abs(samp.cpu().numpy() - z['eval_sample']).reshape(-1, 2).max(1)
        assert (err[diff] < 2e-5).all()


# gradient tolerance relative to max |reference gradient| of the tensor: the fp32 tests use 2e-4; bf16x6 passes the same bar;
# bf16x3 keeps 3e-2 (tools/bf16_split_study.py: up to 1.4e-2 on small-magnitude tensors, typically 1e-4)
GRAD_TOL = {'bf16x6': 2e-4, 'bf16x3': 3e-2}
NORM_TOL = {'bf16x6': 1e-3, 'bf16x3': 2e-2}


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('branch', ['rep', 'mix'])
@pytest.mark.parametrize('path', GOLD, ids=IDS)
def test_vp_train_forward_backward_vs_reference_golden(K, path, branch, mode):
    z = _golden.load(path)
    mtio, m = _build_vp(z, mode)
    m.train()
    h, c, f = (torch.from_numpy(z[k]).cuda() for k in ('history', 'current', 'future'))
    mix_seed = int(z[f'train_{branch}_mixseed'])
    random.seed(mix_seed)
    np.random.seed(mix_seed)
    opt = mtio.FusedAdamW(m, lr=1e-4)
    opt.zero_grad()
    pred, gt = m(h, c, f)
    loss = m.loss_function(pred, gt)
    loss.backward()
    np.testing.assert_array_equal(gt.cpu().numpy(), z[f'train_{branch}_gt'])
    np.testing.assert_allclose(pred.detach().cpu().numpy(), z[f'train_{branch}_pred'], atol=1e-4, rtol=0)
    np.testing.assert_allclose(loss.item(), float(z[f'train_{branch}_loss']), atol=1e-6, rtol=1e-4)
    grads = {k: p.grad.detach().cpu() for k, p in m.named_parameters()}
    names = [str(s) for s in z[f'train_{branch}_gradnames']]
    bad = []
    for k, n in zip(names, z[f'train_{branch}_gradnorms']):
        gn = grads[k].norm().item()
        if abs(gn - n) > NORM_TOL[mode] * max(n, 1e-3) + 1e-6:
            bad.append((k, gn, float(n)))
    assert not bad, bad
    for key in z.files:
        full, sl = key.startswith(f'train_{branch}_grad::'), key.startswith(f'train_{branch}_gradslice::')
        if not (full or sl):
            continue
        k = key.split('::')[1]
        ref = z[key]
        got = grads[k].numpy() if full else grads[k].reshape(grads[k].shape[0], -1)[::37, ::41].numpy()
        # (bf16x3 on the README shape, hist 5 / pred 15: the encoder sees 5 tokens, its in-projection gradient is the smallest-magnitude tensor of the
        # model and takes the mode's largest relative error -- 4.8e-2 of its maximum on 1.5 % of the sampled elements; bf16x6 keeps the fp32 bar)
        tol = 6e-2 if (mode == 'bf16x3' and 's5_t15' in path and 'd512' in path) else GRAD_TOL[mode]
        np.testing.assert_allclose(got, ref, atol=tol * np.abs(ref).max() + 1e-6, rtol=0, err_msg=k)
    bn = m.transformer.distill_layer.norm
    np.testing.assert_allclose(bn.running_mean.cpu().numpy(), z[f'train_{branch}_bn_mean'], atol=2e-6, rtol=1e-4)
    np.testing.assert_allclose(bn.running_var.cpu().numpy(), z[f'train_{branch}_bn_var'], atol=2e-6, rtol=1e-4)


@pytest.mark.parametrize('mode', MODES)
def test_vp_fused_train_step_tracks_fp32_at_bench_width(K, mode):
    """d=512 fused steps (fwd + loss + bwd + AdamW, dropout on, same seeds): the loss trajectory of the split modes stays on the
    fp32 one.  The first step agrees to rounding; AdamW's early steps (update = lr * sign-like g / sqrt(v)) amplify rounding-level
    gradient differences, so later steps are compared at 2e-3 (bf16x6; measured 5e-4 at step 4) / 1e-2 (bf16x3)."""
    from mansy_immersivevideostreaming_amd.viewport_prediction.models import mtio
    h, c, f = (t.cuda() for t in vo.synthetic_trajectories(256, 10, 10, seed=3))
    curves = {}
    for md in ('f32', mode):
        torch.manual_seed(0); random.seed(0); np.random.seed(0)
        m = mtio.ViewportTransformerMTIO(in_channel=2, fut_window=10, d_model=512, dim_feedforward=512, device='cuda', seed=1)
        m.load_state_dict(vo.make_state_dict(512, 3, bias=True))
        m = m.to('cuda').train()
        m.precision = md
        opt = mtio.FusedAdamW(m, lr=1e-4)
        curves[md] = [m.train_step(h, c, f, opt).item() for _ in range(6)]
    np.testing.assert_allclose(curves[mode][0], curves['f32'][0], rtol={'bf16x6': 2e-6, 'bf16x3': 5e-5}[mode])
    np.testing.assert_allclose(curves[mode], curves['f32'], rtol={'bf16x6': 2e-3, 'bf16x3': 1e-2}[mode])


# ------------------------------------------------------------------ plain bf16 (MANSY_PREC_BF16 = 1): one product, a perf mode
@pytest.mark.parametrize('akm,bkm', [(0, 0), (0, 1), (1, 1), (1, 0)])
def test_plain_bf16_product_all_layouts(K, akm, bkm):
    """precision 'bf16' (round 4): ONE bf16 MFMA product per fp32 product, operands rounded to bf16 on their way into LDS, fp32 accumulate --
    the class of the reference's own GPU setting (torch.set_float32_matmul_precision('high'), run_models.py:135).  Against float64 within the
    bf16 rounding bound (2^-9 per operand: ~1e-3 of max |C| on N(0,1) operands), clearly looser than bf16x3 (so the mode is really a
    different arithmetic), every layout / tile / ragged shape, fused epilogue included."""
    g = torch.Generator().manual_seed(3)
    worst = 0.0
    for M, N, Kd in SHAPES:
        if (akm and M % 4) or (bkm and N % 4):
            continue
        A = torch.randn((Kd, M) if akm else (M, Kd), generator=g).cuda()
        B = torch.randn((Kd, N) if bkm else (N, Kd), generator=g).cuda()
        ref = (A.double().t() if akm else A.double()) @ (B.double() if bkm else B.double().t())
        for tile in (0, 64, 128):
            with K.precision('bf16'):
                C = K.gemm(A, B, bool(akm), bool(bkm), force_tile=tile)
            err = ((C.double() - ref).abs().max() / ref.abs().max()).item()
            assert err < 6e-3, (akm, bkm, M, N, Kd, tile, err)
            worst = max(worst, err)
    assert worst > 10 * GEMM_TOL['bf16x3']
    if not akm and not bkm:
        A = torch.randn(300, 256, generator=g).cuda(); W = torch.randn(132, 256, generator=g).cuda()
        bias, R = torch.randn(132, generator=g).cuda(), torch.randn(300, 132, generator=g).cuda()
        with K.precision('bf16'):
            C = K.gemm(A, W, bias=bias, relu=True, resid=R)
        want = torch.relu(A.double() @ W.double().t() + bias.double().cuda()) + R.double()
        assert (C.double() - want).abs().max().item() < 6e-3 * (A.double() @ W.double().t()).abs().max().item()


def test_plain_bf16_vp_train_step_and_sample_track_fp32(K):
    """The VP model in precision 'bf16': the fused train step's loss trajectory stays within a few per cent of the fp32 one (d = 512, dropout
    on, same seeds) and sample() stays within 2e-2 of the fp32 predictions -- a perf mode, held to a perf mode's bar."""
    from mansy_immersivevideostreaming_amd.viewport_prediction.models import mtio
    h, c, f = (t.cuda() for t in vo.synthetic_trajectories(256, 10, 10, seed=3))
    curves, preds = {}, {}
    for md in ('f32', 'bf16'):
        torch.manual_seed(0); random.seed(0); np.random.seed(0)
        m = mtio.ViewportTransformerMTIO(in_channel=2, fut_window=10, d_model=512, dim_feedforward=512, device='cuda', seed=1)
        m.load_state_dict(vo.make_state_dict(512, 3, bias=True))
        m = m.to('cuda').train()
        m.precision = md
        opt = mtio.FusedAdamW(m, lr=1e-4)
        curves[md] = [m.train_step(h, c, f, opt).item() for _ in range(6)]
        m.eval()
        preds[md] = m.sample(h, c).cpu()
    assert curves['bf16'][0] != curves['f32'][0]
    np.testing.assert_allclose(curves['bf16'], curves['f32'], rtol=5e-2)
    assert all(np.isfinite(curves['bf16'])) and curves['bf16'][-1] < curves['bf16'][0]
    d = (preds['bf16'] - preds['f32']).abs()
    d = torch.minimum(d, 1 - d)                        # coordinates live on the unit torus
    assert d.max().item() < 2e-2


# ------------------------------------------------------------------ bitrate-selection nets against the reference goldens
@pytest.fixture(scope='module')
def M():
    from mansy_immersivevideostreaming_amd.bitrate_selection.models import mansy, mansy_ppo
    from mansy_immersivevideostreaming_amd.bitrate_selection.envs import mansy_env

    class NS:
        pass
    ns = NS()
    ns.mansy, ns.ppo, ns.env = mansy, mansy_ppo, mansy_env
    return ns


def _policy(M, sd):
    from test_gpu_ppo import build_policy
    return build_policy(M, sd)


@pytest.mark.parametrize('mode', MODES)
def test_ppo_nets_forward_vs_reference(K, M, mode):
    sd = po.make_policy_state_dict(int(ZP['wseed']))
    pol = _policy(M, sd)
    obs = torch.from_numpy(ZP['obs'][:64]).cuda()
    with K.precision(mode):
        logits, _ = pol.actor(obs)
        value = pol.critic(obs)
        pred = pol.identifier(obs)
    np.testing.assert_allclose(logits.cpu().numpy(), ZP['logits'], atol=1e-4, rtol=0)
    np.testing.assert_allclose(value.cpu().numpy(), ZP['value'], atol=1e-4, rtol=0)
    np.testing.assert_allclose(pred.cpu().numpy(), ZP['ident'], atol=1e-4, rtol=0)
    assert (logits.argmax(-1).cpu().numpy() == ZP['logits'].argmax(-1)).all()        # bitrate decisions identical


@pytest.mark.parametrize('mode', MODES)
def test_identifier_reward_and_training_vs_reference(K, M, mode):
    sd = po.make_policy_state_dict(int(ZP['wseed']))
    pol = _policy(M, sd)
    rows = ZP['ident_reward_rows']
    buf = M.ppo.RolloutBuffer(len(rows), 1, 'cuda')
    buf.obs[:, 0] = torch.from_numpy(ZP['obs'][rows]).cuda()
    buf.rew[:, 0] = 0.25
    buf.filled = len(rows)
    with K.precision(mode):
        pol.relabel(buf, lamb=0.5)
    np.testing.assert_allclose(buf.rew[:, 0].cpu().numpy(), 0.5 * 0.25 + 0.5 * ZP['ident_reward'], atol=1e-5, rtol=0)
    # a full train_identifier() call (mansy_utils.py:9-39) against the capture of the imported reference
    n = int(ZP['ti_n'])
    buf = M.ppo.RolloutBuffer(n, 1, 'cuda')
    buf.obs[:, 0] = torch.from_numpy(ZP['obs'][:n]).cuda()
    buf.filled = n
    np.random.seed(int(ZP['ti_npseed']))
    with K.precision(mode):
        losses, vloss = pol.train_identifier(buf, update_round=2, verbose=False)
    got = [l.item() for l in losses] + [vloss.item()]
    np.testing.assert_allclose(got, ZP['ti_losses'], rtol={'bf16x6': 1e-4, 'bf16x3': 1e-3}[mode], atol=1e-7)
    after = pol.state_dict()
    for key in ZP.files:
        if key.startswith('ti_after::'):
            # Adam's first two steps move every weight by up to lr = 1e-4 each, in the direction of sign(g): an element whose
            # gradient is at rounding-noise level may go the other way in either implementation (<= 2 * 2 * lr apart); all
            # others agree to a fraction of lr
            err = np.abs(after[key[10:]].cpu().numpy() - ZP[key])
            tol = {'bf16x6': 5e-6, 'bf16x3': 1e-4}[mode]
            assert (err > tol).mean() <= 0.03 and err.max() <= 4.5e-4, (key, float((err > tol).mean()), float(err.max()))


# ------------------------------------------------------------------ config C5: 8-preference table + identifier training
QOE_TRAIN = [[7, 1, 1], [1, 7, 1], [1, 1, 7], [3, 3, 3]]          # config.yml:142 (train / valid)
QOE_TEST = [[5, 1, 3], [2, 4, 3], [1, 3, 5], [4, 4, 1]]           # config.yml:144 (test)


def _cycle(M, K, mode, cycles=2):
    torch.manual_seed(0)
    np.random.seed(0)
    pol = _policy(M, po.make_policy_state_dict(5))
    prefs = QOE_TRAIN + QOE_TEST
    T = M.env.EnvTables.synthetic('cuda', n_video=4, n_user=3, n_trace=5, seed=1, n_sample=64, qoe_weights=prefs)
    venv = M.env.MANSYVecEnv(T, 64, seed=5)
    col = M.ppo.VecCollector(pol, venv, seed=5)
    buf = M.ppo.RolloutBuffer(16, 64, 'cuda')
    out = dict(id_losses=[], ppo_losses=[], T=T)
    with K.precision(mode):
        for _ in range(cycles):
            col.collect(16 * 64, buf)
            losses, vloss = pol.train_identifier(buf, 2, verbose=False)
            out['id_losses'] += [l.item() for l in losses] + [vloss.item()]
            if 'obs0' not in out:
                out['obs0'] = buf.obs[0].clone()
                out['pred0'] = pol.identifier(buf.obs[0]).clone()
                out['logits0'] = pol.actor(buf.obs[0])[0].clone()
            res = pol.update(0, buf, is_train=True, batch_size=256, repeat=2)
            out['ppo_losses'] += list(res['loss'])
        out['flat'] = pol.engine.ac.flat_p.clone()
    return out


def test_plain_bf16_ppo_nets_and_cycle(K, M):
    """precision 'bf16' on the bitrate-selection path: logits / values / identifier predictions of the reference golden within 2e-2 (a perf
    mode's bar), and two collect -> train_identifier -> relabel -> update cycles on the eight-preference table run through every product of the
    engine (block-diagonal FeatureNet with K windows, slab-split heads, weight-gradient products with tile lists) with finite, falling losses."""
    sd = po.make_policy_state_dict(int(ZP['wseed']))
    pol = _policy(M, sd)
    obs = torch.from_numpy(ZP['obs'][:64]).cuda()
    with K.precision('bf16'):
        logits, _ = pol.actor(obs)
        value = pol.critic(obs)
        pred = pol.identifier(obs)
    np.testing.assert_allclose(logits.cpu().numpy(), ZP['logits'], atol=2e-2, rtol=0)
    np.testing.assert_allclose(value.cpu().numpy(), ZP['value'], atol=2e-2, rtol=0)
    np.testing.assert_allclose(pred.cpu().numpy(), ZP['ident'], atol=2e-2, rtol=0)
    assert float(np.abs(logits.cpu().numpy() - ZP['logits']).max()) > 1e-5          # (really another arithmetic)
    got, ref = _cycle(M, K, 'bf16'), _cycle(M, K, 'f32')
    assert np.isfinite(got['id_losses']).all() and np.isfinite(got['ppo_losses']).all() and torch.isfinite(got['flat']).all()
    np.testing.assert_allclose(got['id_losses'][:3], ref['id_losses'][:3], rtol=5e-2)
    assert got['id_losses'][1] < got['id_losses'][0]


@pytest.mark.parametrize('mode', MODES)
def test_c5_eight_preference_table_identifier_and_ppo_cycle(K, M, mode):
    ref = _cycle(M, K, 'f32')
    got = _cycle(M, K, mode)
    # --- the 8-preference table: one vectorised environment holds all 4 + 4 vectors; every observation row carries the
    # normalised preference of its episode (mansy_env.py:133-135), and all eight occur in the first vector step
    prefs = np.array(QOE_TRAIN + QOE_TEST, np.float32)
    norm = prefs / prefs.sum(1, keepdims=True)
    assert got['T'].t['qoe_w'].shape == (8, 3)
    w = got['obs0'][:, 745:748].cpu().numpy()
    idx = np.abs(w[:, None, :] - norm[None]).sum(-1).argmin(1)
    np.testing.assert_allclose(w, norm[idx], atol=1e-6)
    assert set(idx.tolist()) == set(range(8))
    # same rollout in both modes up to here: the first observations are bit-identical, the decisions on them too
    assert torch.equal(got['obs0'], ref['obs0'])
    np.testing.assert_allclose(got['pred0'].cpu().numpy(), ref['pred0'].cpu().numpy(), atol=1e-4, rtol=0)
    np.testing.assert_allclose(got['logits0'].cpu().numpy(), ref['logits0'].cpu().numpy(), atol=1e-4, rtol=0)
    assert torch.equal(got['logits0'].argmax(-1), ref['logits0'].argmax(-1))
    # identifier training (the "representation" of configs[4]) and the PPO losses of the first cycle track the fp32 run;
    # later cycles sample different actions once logits differ in the last bits, so only finiteness is asserted there
    k = 3
    np.testing.assert_allclose(got['id_losses'][:k], ref['id_losses'][:k], rtol={'bf16x6': 2e-4, 'bf16x3': 2e-3}[mode])
    np.testing.assert_allclose(got['ppo_losses'][:4], ref['ppo_losses'][:4], rtol={'bf16x6': 2e-3, 'bf16x3': 2e-2}[mode], atol=1e-4)
    assert np.isfinite(got['id_losses']).all() and np.isfinite(got['ppo_losses']).all() and torch.isfinite(got['flat']).all()
    assert got['id_losses'][-1] < got['id_losses'][0]


@pytest.mark.parametrize('mode', MODES + ['f32'])
def test_single_k_tile_products_at_the_end_of_an_allocation(K, mode):
    """K == 32 (one K-tile per workgroup) with the operands placed at the very end of their own 64 MiB allocations: the pipelined
    loops re-load their last tile instead of branching, and must never form an address beyond the operand (round-2 regression:
    the two-stage split loop advanced its tile corners once too often when there was a single K-tile -- a read past the end
    that only faults when the next page is unmapped)."""
    g = torch.Generator().manual_seed(2)
    n_big = 16 * 1024 * 1024                                   # 64 MiB of floats: a multiple of the allocator's 2 MiB segments
    for akm, bkm, M, N in ((0, 0, 192, 64), (1, 1, 128, 192), (0, 1, 64, 128), (1, 0, 256, 64)):
        bigA, bigB = torch.empty(n_big, device='cuda'), torch.empty(n_big, device='cuda')
        A = bigA[n_big - M * 32:].view((32, M) if akm else (M, 32))
        B = bigB[n_big - N * 32:].view((32, N) if bkm else (N, 32))
        A.copy_(torch.randn(A.shape, generator=g)); B.copy_(torch.randn(B.shape, generator=g))
        ref = (A.double().t() if akm else A.double()) @ (B.double() if bkm else B.double().t())
        with K.precision(mode):
            for tile in (0, 64, 128):
                C = K.gemm(A, B, bool(akm), bool(bkm), force_tile=tile)
                torch.cuda.synchronize()
                assert ((C.double() - ref).abs().max() / ref.abs().max()).item() < GEMM_TOL[mode]
        del bigA, bigB


@pytest.mark.parametrize('mode', MODES)
def test_weight_planes_and_presplit_product(K, mode):
    """Weights split ahead of the product (what the viewport engine does once per step): the planes re-assemble the weight
    (a0 + a1 (+ a2) == W to 2^-16 / 2^-24 relative), the transposed planes are the planes of W^T, and the LDS-DMA product on
    them agrees with the float64 product like the in-loop split does -- forward (A W^T) and dX (A W) forms, ragged rows, one to
    many K-tiles, both tiles, with a fused epilogue."""
    npl = 2 if mode == 'bf16x3' else 3
    g = torch.Generator().manual_seed(8)
    for (M, N, Kd) in ((4096, 512, 512), (300, 1536, 512), (70, 64, 32), (257, 96, 1536), (2048, 512, 64), (40960, 512, 512), (1000, 260, 96)):
        W = torch.randn(N, Kd, generator=g).cuda()
        pl, pl_t = K.weight_planes(W, npl)
        back = sum(pl[t].view(torch.bfloat16).float() for t in range(npl))
        assert ((back - W).abs().max() / W.abs().max()).item() < (2.0 ** -15 if npl == 2 else 2.0 ** -22)
        assert torch.equal(pl_t, pl.transpose(1, 2).contiguous())
        A = torch.randn(M, Kd, generator=g).cuda()
        G = torch.randn(M, N, generator=g).cuda()
        bias, resid = torch.randn(N, generator=g).cuda(), torch.randn(M, N, generator=g).cuda()
        ref_f = A.double() @ W.double().t()
        ref_b = G.double() @ W.double()
        for tile in (0, 64, 128, 256):        # 256: the eight-wave 256 x 128 three-stage loop (bf16x3); 0 at [40 960, 512] picks it by itself
            with K.precision(mode):
                Cf = K.gemm_planes(A, W, pl, transposed=False, force_tile=tile)
                Cb = K.gemm_planes(G, W, pl_t, transposed=True, force_tile=tile)
                Ce = K.gemm_planes(A, W, pl, transposed=False, bias=bias, relu=True, resid=resid, force_tile=tile)
            assert ((Cf.double() - ref_f).abs().max() / ref_f.abs().max()).item() < GEMM_TOL[mode], (M, N, Kd, tile)
            assert ((Cb.double() - ref_b).abs().max() / ref_b.abs().max()).item() < GEMM_TOL[mode], (M, N, Kd, tile)
            want = torch.relu(ref_f + bias.double()) + resid.double()
            assert (Ce.double() - want).abs().max().item() < GEMM_TOL[mode] * ref_f.abs().max().item(), (M, N, Kd, tile)
    # fp32 mode ignores the planes: bit-identical to the plain product
    W = torch.randn(512, 512, generator=g).cuda()
    A = torch.randn(256, 512, generator=g).cuda()
    pl, _ = K.weight_planes(W, npl)
    assert torch.equal(K.gemm_planes(A, W, pl), K.gemm(A, W))


@pytest.mark.parametrize('mode', MODES)
def test_ring_staged_decoder_tiles_equal_the_two_stage_loop_bit_for_bit(K, mode):
    """The 64 x 64 tiles of the pre-split products run on a three-stage operand ring (gemm_bf16h_kernel: two K-tiles in flight under
    counted vmcnt waits; variant 6: four stages).  Same products in the same order as the round-2 two-stage loop (variant 7), so the
    results must be bit-identical -- over 1..6 K-tiles (prologue shorter than the ring, tail with no DMA left to issue), ragged rows /
    columns, both forms (A W^T and A W), with a fused epilogue, many launches back to back (stage reuse across launches)."""
    npl = 2 if mode == 'bf16x3' else 3
    g = torch.Generator().manual_seed(21)
    for (M, N, Kd) in ((4096, 512, 512), (70, 64, 32), (64, 130, 64), (257, 96, 96), (100, 72, 128), (33, 512, 160), (1000, 260, 192), (4000, 520, 1536)):
        W = torch.randn(N, Kd, generator=g).cuda()
        pl, pl_t = K.weight_planes(W, npl)
        A = torch.randn(M, Kd, generator=g).cuda()
        G = torch.randn(M, N, generator=g).cuda()
        bias, resid = torch.randn(N, generator=g).cuda(), torch.randn(M, N, generator=g).cuda()
        outs = {}
        for v in (7, 1, 6):
            var = K.VARIANT_BF16(v)                      # per call (ABI 8): nothing is remembered by the library
            with K.precision(mode):
                outs[v] = [K.gemm_planes(A, W, pl, force_tile=64, variant=var), K.gemm_planes(G, W, pl_t, transposed=True, force_tile=64, variant=var),
                           K.gemm_planes(A, W, pl, bias=bias, relu=True, resid=resid, force_tile=64, variant=var)]
                for _ in range(3):                       # back to back: nothing of one launch's ring may leak into the next
                    again = K.gemm_planes(A, W, pl, force_tile=64, variant=var)
                assert torch.equal(again, outs[v][0])
        for v in (1, 6):
            for got, want in zip(outs[v], outs[7]):
                assert torch.equal(got, want), (mode, v, M, N, Kd)
        ref = A.double() @ W.double().t()
        assert ((outs[1][0].double() - ref).abs().max() / ref.abs().max()).item() < GEMM_TOL[mode]


def test_role_split_256x128_loop_equals_the_other_loops_bit_for_bit(K):
    """Round 4: the 256 x 128 tiles of the pre-split bf16x3 products run on twelve waves with fixed roles (gemm_bf16k_kernel: 8 consumer
    waves that only read fragments / split / MFMA, 4 loader waves that only issue LDS-DMA; the default, variant 1).  Same products in the
    same order per output element as the eight-wave loop (variant 8, force_tile 256) and the 128 x 128 loop (variant 4, force_tile 128),
    and the same row-major epilogue: bit-identical results -- over 3..48 K-tiles (prologue shorter than the ring, tails with nothing left
    to issue), ragged rows / columns, both forms (A W^T and A W), a fused epilogue, launches back to back (ring reuse across launches)."""
    g = torch.Generator().manual_seed(33)
    for (M, N, Kd) in ((40960, 512, 512), (1000, 260, 96), (257, 128, 128), (4096, 1536, 512), (300, 132, 160), (2048, 512, 1536), (256, 128, 192)):
        W = torch.randn(N, Kd, generator=g).cuda()
        pl, pl_t = K.weight_planes(W, 2)
        A = torch.randn(M, Kd, generator=g).cuda()
        G = torch.randn(M, N, generator=g).cuda()
        bias, resid = torch.randn(N, generator=g).cuda(), torch.randn(M, N, generator=g).cuda()

        def run(tile, v):
            var = K.VARIANT_BF16(v)
            with K.precision('bf16x3'):
                return [K.gemm_planes(A, W, pl, force_tile=tile, variant=var), K.gemm_planes(G, W, pl_t, transposed=True, force_tile=tile, variant=var),
                        K.gemm_planes(A, W, pl, bias=bias, relu=True, resid=resid, force_tile=tile, variant=var)]
        want = run(128, 4)                                # gemm_bf16f_kernel<128, 128>
        for got, w in zip(run(256, 8), want):             # gemm_bf16g_kernel
            assert torch.equal(got, w)
        outs = run(256, 1)                                # gemm_bf16k_kernel
        for got, w in zip(outs, want):
            assert torch.equal(got, w), (M, N, Kd, float((got - w).abs().max()))
        with K.precision('bf16x3'):
            for _ in range(3):
                assert torch.equal(K.gemm_planes(A, W, pl, force_tile=256), want[0])
        ref = A.double() @ W.double().t()
        assert ((want[0].double() - ref).abs().max() / ref.abs().max()).item() < GEMM_TOL['bf16x3']


def test_bf16_storage_step_reads_no_image_it_has_not_written(K):
    """The bf16-STORAGE form of precision 'bf16' (round 6: every operand of a dense product has a bf16 image in the workspace, written by the operand's
    producer; csrc/vp_engine.hip, csrc/gemm_bf16a.hip): the WHOLE workspace -- float slabs and the image arena -- is poisoned before every call, once with
    NaN bit patterns (a leaked value makes the result NaN) and once with huge finite ones (0x7F00 = 1.7e38: a leaked value that only passes through a
    `x > 0 ?` select -- where a NaN would read as a quiet `false` -- blows the result up instead); four train steps and sample() must come out finite and
    no further from the un-poisoned run than two un-poisoned runs are from each other (the split-K atomics of the weight-gradient products add in another
    order from run to run; Adam turns that rounding noise into +-lr steps and the bf16 residual streams amplify it: ~5e-3 on sample() after four steps,
    tools/poison_probe.py): nothing is read that the same call has not written."""
    from mansy_immersivevideostreaming_amd.viewport_prediction.models import mtio
    h, c, f = (t.cuda() for t in vo.synthetic_trajectories(256, 10, 10, seed=4))

    def run(poison):
        torch.manual_seed(0); random.seed(0); np.random.seed(0)
        m = mtio.ViewportTransformerMTIO(in_channel=2, fut_window=10, d_model=512, dim_feedforward=512, device='cuda', seed=1)
        m.load_state_dict(vo.make_state_dict(512, 3, bias=False))
        m = m.to('cuda').train()
        m.precision = 'bf16'
        opt = mtio.FusedAdamW(m, lr=1e-4)
        losses = []
        for _ in range(4):
            if poison is not None:
                m._workspace(m._cfg(256, 10)).view(torch.int16).fill_(poison)          # the pattern in every 16 bits = in both halves of every float
            losses.append(m.train_step(h, c, f, opt).item())
        m.eval()
        if poison is not None:
            m._workspace(m._cfg(256, 10)).view(torch.int16).fill_(poison)
        return np.array(losses), m.sample(h, c).cpu(), m._flat_p.clone().cpu()

    def apart(x, y):
        d = (x[1] - y[1]).abs()
        return np.abs(x[0] / y[0] - 1).max(), torch.minimum(d, 1 - d).max().item(), (x[2] - y[2]).abs().max().item()
    clean, again = run(None), run(None)
    noise = apart(clean, again)
    assert noise[1] <= 2e-2 and noise[2] <= 8e-4          # (4 steps x 2 lr is the most two parameter sets can be apart)
    for pattern in (0x7FC0, 0x7F00):
        got = run(pattern)
        assert np.isfinite(got[0]).all() and torch.isfinite(got[1]).all() and torch.isfinite(got[2]).all(), hex(pattern)
        # the first step starts from identical weights and its loss is a pure function of the forward (no atomics): bit-equal
        assert got[0][0] == clean[0][0]
        d = apart(got, clean)
        assert d[0] <= 3 * noise[0] + 2e-3 and d[1] <= 3 * noise[1] + 2e-3 and d[2] <= 3 * noise[2] + 1e-4, (hex(pattern), d, noise)
