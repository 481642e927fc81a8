"""GPU parity of the individual HIP kernels (through the C ABI) against fp64 torch references / the C
oracle on seeded inputs.  Tolerances are written next to each check; integer work is bit-exact."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import rng as orng  # noqa: E402

G = os.path.join(os.path.dirname(__file__), 'golden')


@pytest.fixture(scope='module')
def K():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a ROCm device (no CPU fallback exists)')
    from mansy_immersivevideostreaming_amd import kernels
    return kernels


def _gemm_ref(A, B, a_kmajor, b_kmajor):
    A64 = A.double().cpu()
    B64 = B.double().cpu()
    Al = A64.t() if a_kmajor else A64
    Bl = B64 if b_kmajor else B64.t()
    ref = Al @ Bl
    bound = (Al.abs() @ Bl.abs())
    return ref, bound


@pytest.mark.parametrize('a_kmajor,b_kmajor', [(False, False), (False, True), (True, True), (True, False)])
@pytest.mark.parametrize('M,N,K_', [(320, 512, 512), (4096, 1536, 512), (257, 130, 70), (64, 64, 32), (1000, 512, 1536), (33, 6, 5), (260, 132, 96), (4, 4, 32)])
@pytest.mark.parametrize('tile', [0, 64, 96, 128, -64, -128])    # 96 = 128x64; negative = register-staged loop (the LDS-DMA loop serves aligned K % 32 == 0 shapes)
def test_gemm_layouts(K, a_kmajor, b_kmajor, M, N, K_, tile):
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K_)
    A = torch.randn((K_, M) if a_kmajor else (M, K_), generator=g).cuda()
    B = torch.randn((K_, N) if b_kmajor else (N, K_), generator=g).cuda()
    out = K.gemm(A, B, a_kmajor, b_kmajor, force_tile=tile)
    ref, bound = _gemm_ref(A, B, a_kmajor, b_kmajor)
    err = (out.double().cpu() - ref).abs()
    # exact-fp32 MFMA chain: error << 2e-6 * sum|a||b| (30 ulp of the absolute-value product)
    assert (err <= 2e-6 * bound + 1e-7).all(), float((err / (bound + 1e-30)).max())


def test_gemm_epilogue_bias_relu_resid_mask(K):
    g = torch.Generator().manual_seed(1)
    M, N, Kd = 300, 512, 512
    A = torch.randn(M, Kd, generator=g).cuda()
    W = torch.randn(N, Kd, generator=g).cuda() * 0.05
    bias = torch.randn(N, generator=g).cuda()
    R = torch.randn(M, N, generator=g).cuda()
    H = torch.randn(M, N, generator=g).cuda()
    ref = (A.double() @ W.double().t() + bias.double())
    out = K.gemm(A, W, bias=bias, relu=True, resid=R)
    torch.testing.assert_close(out.double(), torch.relu(ref) + R.double(), rtol=0, atol=2e-5)
    out = K.gemm(A, W, mask_src=H, mask_scale=1.25)
    exp = torch.where(H > 0, (A.double() @ W.double().t()) * 1.25, torch.zeros_like(ref))
    torch.testing.assert_close(out.double(), exp, rtol=0, atol=2e-5)


def test_gemm_epilogue_dropout_matches_shared_hash(K):
    g = torch.Generator().manual_seed(2)
    M, N, Kd = 130, 192, 64
    A = torch.randn(M, Kd, generator=g).cuda()
    W = torch.randn(N, Kd, generator=g).cuda()
    p, seed, site = 0.1, 1234, 105
    out = K.gemm(A, W, drop=(p, seed, site))
    keep = torch.from_numpy(orng.keep_mask(seed, site, M * N, p)).reshape(M, N).cuda()
    exp = torch.where(keep, (A.double() @ W.double().t()) / (1 - p), torch.zeros(M, N, dtype=torch.float64, device='cuda'))
    torch.testing.assert_close(out.double(), exp, rtol=0, atol=2e-5)
    frac = keep.float().mean().item()
    assert abs(frac - 0.9) < 0.01


@pytest.mark.parametrize('M,N,Kd,bk', [(256, 1280, 320, 0), (512, 1280, 256, 1), (300, 132, 64, 1), (33, 36, 32, 0), (512, 256, 1280, 0), (100, 64, 96, 0)])
def test_wave_split_k_loop_vs_the_64x64_loop(K, M, N, Kd, bk):
    """Round 4: fp32 products too small to fill the chip (<= 200 tiles of 64 x 64) run on gemm_f32_wsk_kernel -- 32 x 32 blocks, the four waves of a
    workgroup split the K-tiles, partial blocks added in wave order.  Same product, another (deterministic) summation order: against the 64 x 64
    loop (knob off) to fp32 rounding, against float64 within the exact-fp32 bound, with every fused epilogue, ragged rows / columns, K-major B,
    1..40 K-tiles (waves with no tile at all), run to run bit-identical."""
    g = torch.Generator().manual_seed(M + N + Kd)
    A = torch.randn(M, Kd, generator=g).cuda()
    B = torch.randn((Kd, N) if bk else (N, Kd), generator=g).cuda()
    bias = torch.randn(N, generator=g).cuda()
    R = torch.randn(M, N, generator=g).cuda()
    H = torch.randn(M, N, generator=g).cuda()
    outs = {}
    for v in (0, 1):          # ABI 8: the loop is chosen per call (mansy_gemm_epilogue::variant), there is no process-wide knob
        var = 0 if v else K.VARIANT_NO_WSK
        outs[v] = [K.gemm(A, B, False, bool(bk), force_tile=64, variant=var),
                   K.gemm(A, B, False, bool(bk), bias=bias, relu=True, resid=R, force_tile=64, variant=var),
                   K.gemm(A, B, False, bool(bk), mask_src=H, mask_scale=1.25, force_tile=64, variant=var),
                   K.gemm(A, B, False, bool(bk), drop=(0.1, 77, 5), force_tile=64, variant=var)]
    assert torch.equal(K.gemm(A, B, False, bool(bk), force_tile=64), outs[1][0])          # deterministic
    ref, bound = _gemm_ref(A, B, False, bool(bk))
    err = (outs[1][0].double().cpu() - ref).abs()
    assert (err <= 2e-6 * bound + 1e-7).all()
    scale = float(ref.abs().max())
    for a, b in zip(outs[0], outs[1]):
        assert (a - b).abs().max().item() <= 4e-6 * scale
    if M * N <= 64 * 64 * 200 and not bk and Kd % 32 == 0 and M >= 64:       # the two loops really are different loops: another summation order
        assert any(not torch.equal(a, b) for a, b in zip(outs[0], outs[1])) or Kd <= 32


def test_gemm_splitk_accumulate(K):
    g = torch.Generator().manual_seed(3)
    rows, N, Kd = 40960 // 4, 512, 512                  # dW = dY^T X over many rows
    dY = torch.randn(rows, N, generator=g).cuda()
    X = torch.randn(rows, Kd, generator=g).cuda()
    out = torch.ones(N, Kd, device='cuda')
    K.gemm(dY, X, a_kmajor=True, b_kmajor=True, out=out, accumulate=True)
    ref = dY.double().t() @ X.double() + 1.0
    bound = dY.double().abs().t() @ X.double().abs()
    err = (out.double() - ref).abs()
    assert (err <= 2e-6 * bound + 1e-6).all()


@pytest.mark.parametrize('rows,accumulate', [(3276, True), (3276, False), (300, False), (1028, True)])
def test_gemm_long_k_with_tail(K, rows, accumulate):
    """Reduce dimension not a multiple of the K-tile: whole K-tiles on the LDS-DMA loop + the leftover rows as a second,
    accumulating launch (the PPO identifier's dW over int(0.8 * 4096) = 3276 transitions)."""
    g = torch.Generator().manual_seed(rows)
    dY = torch.randn(rows, 128, generator=g).cuda()
    X = torch.randn(rows, 764, generator=g).cuda()
    out = torch.full((128, 764), 0.5, device='cuda')
    K.gemm(dY, X, a_kmajor=True, b_kmajor=True, out=out, accumulate=accumulate)
    ref = dY.double().t() @ X.double() + (0.5 if accumulate else 0.0)
    bound = dY.double().abs().t() @ X.double().abs()
    assert ((out.double() - ref).abs() <= 2e-6 * bound + 1e-6).all()
    # K-contiguous operands too
    A = torch.randn(200, rows, generator=g).cuda()
    W = torch.randn(96, rows, generator=g).cuda()
    o2 = K.gemm(A, W)
    r2 = A.double() @ W.double().t()
    assert ((o2.double() - r2).abs() <= 2e-6 * (A.double().abs() @ W.double().abs().t()) + 1e-6).all()


@pytest.mark.parametrize('B,L,d,H', [(5, 10, 512, 8), (3, 16, 64, 8), (7, 5, 128, 8), (2, 1, 512, 8), (9, 5, 512, 8), (4, 2, 512, 8), (3, 7, 256, 4), (2, 12, 512, 8),
                                     (5, 3, 512, 8), (5, 4, 512, 8), (5, 6, 512, 8), (5, 8, 512, 8), (5, 9, 512, 8)])
@pytest.mark.parametrize('p', [0.0, 0.1])
def test_attention_fwd_bwd(K, B, L, d, H, p):
    g = torch.Generator().manual_seed(L * 100 + d)
    qkv = torch.randn(B, L, 3 * d, generator=g).cuda()
    dout = torch.randn(B, L, d, generator=g).cuda()
    drop = (p, 77, 100)
    out, P = K.attn_fwd_packed(qkv, H, drop=drop)
    dqkv = K.attn_bwd_packed(qkv, P, dout, H, drop=drop)
    # fp64 torch reference with the same (shared-hash) dropout mask
    x = qkv.double().cpu().requires_grad_(True)
    dh = d // H
    q, k, v = x.split(d, dim=-1)
    qh, kh, vh = (t.reshape(B, L, H, dh).permute(0, 2, 1, 3) for t in (q, k, v))
    Pr = torch.softmax(qh @ kh.transpose(-1, -2) / dh ** 0.5, dim=-1)
    keep = torch.from_numpy(orng.keep_mask(77, 100, B * H * L * L, p)).reshape(B, H, L, L).double()
    o = ((Pr * keep / (1 - p)) @ vh).permute(0, 2, 1, 3).reshape(B, L, d)
    o.backward(dout.double().cpu())
    torch.testing.assert_close(P.double().cpu().reshape(B, H, L, L), Pr.detach(), rtol=0, atol=2e-6)
    torch.testing.assert_close(out.double().cpu(), o.detach(), rtol=0, atol=2e-5)
    torch.testing.assert_close(dqkv.double().cpu(), x.grad, rtol=0, atol=5e-5)


@pytest.mark.parametrize('rows,C', [(1000, 512), (33, 64), (4096, 256), (7, 1024), (10, 96)])
@pytest.mark.parametrize('with_b,with_bias', [(True, True), (False, False)])
def test_layernorm_fwd_bwd(K, rows, C, with_b, with_bias):
    g = torch.Generator().manual_seed(rows + C)
    a = torch.randn(rows, C, generator=g).cuda()
    b = torch.randn(rows, C, generator=g).cuda() if with_b else None
    w = (1 + 0.1 * torch.randn(C, generator=g)).cuda()
    bias = torch.randn(C, generator=g).cuda() if with_bias else None
    dy = torch.randn(rows, C, generator=g).cuda()
    y, z, mean, rstd = K.layernorm_fwd(a, b, w, bias)
    zr = (a.double() + (b.double() if with_b else 0)).cpu().requires_grad_(True)
    wr = w.double().cpu().requires_grad_(True)
    br = bias.double().cpu().requires_grad_(True) if with_bias else None
    yr = torch.nn.functional.layer_norm(zr, (C,), wr, br, 1e-5)
    yr.backward(dy.double().cpu())
    torch.testing.assert_close(y.double().cpu(), yr.detach(), rtol=0, atol=5e-6)
    torch.testing.assert_close(z.double().cpu(), zr.detach(), rtol=0, atol=1e-6)
    dz, dz_drop, dw, db = K.layernorm_bwd(dy, z, mean, rstd, w, drop=(0.1, 9, 3), want_bias=with_bias)
    torch.testing.assert_close(dz.double().cpu(), zr.grad, rtol=0, atol=2e-5)
    tol = 1e-5 * rows ** 0.5 + 1e-5
    torch.testing.assert_close(dw.double().cpu(), wr.grad, rtol=0, atol=tol * 4)
    if with_bias:
        torch.testing.assert_close(db.double().cpu(), br.grad, rtol=0, atol=tol * 4)
    keep = torch.from_numpy(orng.keep_mask(9, 3, rows * C, 0.1)).reshape(rows, C).cuda()
    torch.testing.assert_close(dz_drop, torch.where(keep, dz / 0.9, torch.zeros_like(dz)), rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize('rows,C', [(4096, 512), (300, 256), (40, 512), (5000, 1024)])
def test_layernorm_bwd_partial_matches_atomic_form(K, rows, C):
    """Engine form (per-workgroup partial sums + reduce, accumulated over two 'steps') == two atomic-form calls."""
    g = torch.Generator().manual_seed(rows * 3 + C)
    w = (1 + 0.1 * torch.randn(C, generator=g)).cuda()
    dw_ref = torch.zeros(C, device='cuda', dtype=torch.float64); db_ref = torch.zeros_like(dw_ref)
    partials = None
    for step in range(2):
        a = torch.randn(rows, C, generator=g).cuda()
        dy = torch.randn(rows, C, generator=g).cuda()
        _, z, mean, rstd = K.layernorm_fwd(a, None, w, None)
        drop = (0.1, 11, 40 + step)
        dz0, dzd0, dw0, db0 = K.layernorm_bwd(dy, z, mean, rstd, w, drop=drop)
        dz1, dzd1, partials = K.layernorm_bwd_partial(dy, z, mean, rstd, w, drop=drop, partials=partials, accumulate=step > 0)
        assert torch.equal(dz0, dz1) and torch.equal(dzd0, dzd1)        # same row arithmetic, bit for bit
        dw_ref += dw0.double(); db_ref += db0.double()
    dw = torch.ones(C, device='cuda'); db = torch.full((C,), 2.0, device='cuda')
    K.ln_partials_reduce(partials, dw, db)
    tol = 1e-5 * (2 * rows) ** 0.5 + 1e-5
    torch.testing.assert_close(dw.double() - 1.0, dw_ref, rtol=0, atol=tol * 4)
    torch.testing.assert_close(db.double() - 2.0, db_ref, rtol=0, atol=tol * 4)


@pytest.mark.parametrize('T,B,M,p', [(10, 37, 5, 0.1), (3, 8, 1, 0.0), (16, 5, 16, 0.1), (1, 4, 7, 0.1)])
def test_attn_cross_deferred_kv_grads_match_stepwise(K, T, B, M, p):
    """dK/dV of the memory from one deferred pass == T accumulating read-modify-write passes; dQ identical."""
    H, d = 8, 512
    g = torch.Generator().manual_seed(T * 100 + B + M)
    q = torch.randn(T, B, d, generator=g).cuda()
    dO = torch.randn(T, B, d, generator=g).cuda()
    memkv = torch.randn(B, M, 2 * d, generator=g).cuda()
    P = torch.softmax(torch.randn(T, B * H, M, generator=g), dim=-1).cuda()
    sites = [10000 + 8 * i + 2 for i in range(T)]
    dq0, dkv0 = K.attn_cross_stepwise(q, memkv, P, dO, H, sites, p, 123)
    dq1, dkv1 = K.attn_cross_deferred(q, memkv, P, dO, H, sites, p, 123)
    assert torch.equal(dq0, dq1)
    torch.testing.assert_close(dkv1, dkv0, rtol=1e-5, atol=2e-5)
    # and against fp64 autograd for one configuration
    if T == 10:
        keep = torch.stack([torch.from_numpy(orng.keep_mask(123, sites[i], B * H * M, p)).reshape(B * H, M) for i in range(T)]).cuda().double()
        kv = memkv.double().clone().requires_grad_(True)
        Kh = kv[:, :, :d].reshape(B, M, H, 64).permute(0, 2, 1, 3)         # [B,H,M,64]
        Vh = kv[:, :, d:].reshape(B, M, H, 64).permute(0, 2, 1, 3)
        qh = q.double().reshape(T, B, H, 1, 64).requires_grad_(True)
        sc = (qh @ Kh.transpose(-1, -2)) / 8.0                              # [T,B,H,1,M]
        Pr = torch.softmax(sc, dim=-1)
        o = ((Pr * keep.reshape(T, B, H, 1, M) / (1 - p)) @ Vh).reshape(T, B, d)
        # the kernels take P as given; use the same P by feeding the softmax of these scores back in
        Pin = Pr.detach().reshape(T, B * H, M).float()
        dq2, dkv2 = K.attn_cross_deferred(q, memkv, Pin, dO, H, sites, p, 123)
        o.backward(dO.double())
        torch.testing.assert_close(dkv2.double(), kv.grad, rtol=0, atol=5e-5)
        torch.testing.assert_close(dq2.double(), qh.grad.reshape(T, B, d), rtol=0, atol=5e-5)


@pytest.mark.parametrize('T,B,p', [(10, 33, 0.1), (4, 8, 0.0), (16, 5, 0.1), (1, 4, 0.1)])
def test_attn_self_decode_pull_matches_stepwise(K, T, B, p):
    """Pull-form self-attention backward (each K/V gradient row written once) == the read-modify-write form."""
    H, d = 8, 512
    g = torch.Generator().manual_seed(T * 10 + B)
    qkv = torch.randn(T, B, 3 * d, generator=g).cuda()
    dO = torch.randn(T, B, d, generator=g).cuda()
    P = torch.zeros(T, B * H, T)
    for i in range(T):        # row i: i+1 probabilities per (batch, head), packed with stride i+1 at the start of the step's block
        pi = torch.softmax(torch.randn(B * H, i + 1, generator=g), dim=-1)
        P[i].view(-1)[:B * H * (i + 1)] = pi.reshape(-1)
    P = P.cuda()
    sites = [10000 + 8 * i for i in range(T)]
    ref = K.attn_self_decode_bwd(qkv, P, dO, H, sites, p, 321, pull=False)
    got = K.attn_self_decode_bwd(qkv, P, dO, H, sites, p, 321, pull=True)
    torch.testing.assert_close(got, ref, rtol=1e-5, atol=2e-5)


def test_tilemap_bit_exact_vs_oracle_and_reference_goldens(K):
    from oracle import tilemap as tm
    z = np.load(os.path.join(G, 'tilemap_px.npz'))
    px = z['px'].astype(np.float64)
    # pixel grid -> normalised coords that truncate back to the same pixel: (px + 0.5) / size
    xy = np.stack([(px[:, 0] + 0.5) / 2560.0, (px[:, 1] + 0.5) / 1440.0], 1).astype(np.float32)
    back = np.stack([(xy[:, 0] * np.float32(2560)).astype(np.int32), (xy[:, 1] * np.float32(1440)).astype(np.int32)], 1)
    sel = (back == z['px']).all(1)
    got = K.tilemap(torch.from_numpy(xy).cuda()).cpu().numpy().view(np.uint64)
    np.testing.assert_array_equal(got[sel], z['maps'][sel])
    assert sel.sum() > 5000
    # dataset traces: gt maps of the reference's shipped prediction pickles, via per-chunk OR on device
    zd = np.load(os.path.join(G, 'tilemap_dataset.npz'))
    for v, u in zd['pairs']:
        tr = zd[f'trace_{v}_{u}']
        ts = list(range(15, len(tr) - 15, 5))
        fut = np.stack([tr[t + 1:t + 6] for t in ts])                       # [n,5,2]
        maps = K.tilemap(torch.from_numpy(fut).cuda())
        ored = K.tilemap_or_groups(maps.reshape(-1), 5)
        np.testing.assert_array_equal(tm.bits_to_u8(ored.cpu().numpy().view(np.uint64)), zd[f'gt_{v}_{u}'])
        pred_bits = (zd[f'pred_{v}_{u}'].astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(1).astype(np.uint64)
        iou = K.tilemap_iou(ored, torch.from_numpy(pred_bits.view(np.int64)).cuda())
        np.testing.assert_allclose(iou.cpu().numpy(), zd[f'iou_{v}_{u}'], rtol=0, atol=1e-12)
    # random points incl. edges, against the C oracle
    rs = np.random.RandomState(0)
    xy = rs.rand(200000, 2).astype(np.float32)
    xy[:100] = 0.0
    xy[100:200] = 1.0
    got = K.tilemap(torch.from_numpy(xy).cuda()).cpu().numpy().view(np.uint64)
    np.testing.assert_array_equal(got, tm.tilemap_xy(xy))


@pytest.mark.parametrize('geom', [(2560, 1440, 8, 8, 600, 300), (1920, 1080, 6, 4, 400, 200), (3840, 1920, 16, 4, 1000, 500),
                                  (1280, 720, 4, 4, 600, 300), (2560, 1440, 32, 2, 90, 90)])
def test_tilemap_other_geometries_and_every_wrap_case_vs_oracle(K, geom):
    """The generic kernel (run-time frame / grid / FoV) and the constant-folded standard one against the C oracle: a dense sweep of the
    frame borders, every tile boundary +-1 pixel, both axes, so that all nine region cases of _find_regions_covered_by_fov
    (viewport_prediction/utils/common.py:83-127) and the "exact multiple belongs to the lower tile" rule occur."""
    from oracle import tilemap as tm
    W, H, nw, nh, fw, fh = geom
    tw, th = W // nw, H // nh
    xs = sorted({v for k in range(nw + 1) for v in (k * tw - 1, k * tw, k * tw + 1)} | {fw // 2 - 1, fw // 2, fw // 2 + 1, W - fw // 2 - 1,
                 W - fw // 2, W - fw // 2 + 1} | set(range(0, W + 1, max(1, W // 97))))
    ys = sorted({v for k in range(nh + 1) for v in (k * th - 1, k * th, k * th + 1)} | {fh // 2 - 1, fh // 2, fh // 2 + 1, H - fh // 2 - 1,
                 H - fh // 2, H - fh // 2 + 1} | set(range(0, H + 1, max(1, H // 89))))
    xs = [x for x in xs if 0 <= x <= W]
    ys = [y for y in ys if 0 <= y <= H]
    px = np.array([(x, y) for x in xs for y in ys], np.int64)
    xy = np.stack([(px[:, 0] + 0.5) / W, (px[:, 1] + 0.5) / H], 1).astype(np.float32)
    xy[px[:, 0] == W, 0] = 1.0
    xy[px[:, 1] == H, 1] = 1.0
    back = np.stack([(xy[:, 0] * np.float32(W)).astype(np.int32), (xy[:, 1] * np.float32(H)).astype(np.int32)], 1)
    assert (back == px).mean() > 0.99
    got = K.tilemap(torch.from_numpy(xy).cuda(), W, H, nw, nh, fw, fh).cpu().numpy().view(np.uint64)
    want = tm.tilemap_xy(xy, W, H, nw, nh, fw, fh)
    np.testing.assert_array_equal(got, want)
    assert len(np.unique(want)) > 4 * max(nw, nh) // 2


def test_tilemap_centres_outside_the_frame_vs_imported_reference(K):
    """Raw predictions reach the tile map (predict.py:40-45, results.py:15-18), and the linear-regression baseline extrapolates across
    wrap-around jumps, so centres far outside the frame occur: Python floor division on negative pixels and numpy's slice semantics
    on negative tile indices (a negative stop counts from the end of the axis) are part of the reference's behaviour.  9 165 such
    centres through the imported function (tools/gen_golden_tilemap_outside.py) against the kernel and the C oracle, bit-exact."""
    from oracle import tilemap as tm
    z = np.load(os.path.join(G, 'tilemap_px_outside.npz'))
    assert not z['raised'].any()
    px = z['px'].astype(np.float64)
    # a normalised coordinate that truncates (toward zero, like int()) back to the pixel: centre of the pixel's unit interval
    xy = np.stack([(px[:, 0] + np.where(px[:, 0] >= 0, 0.5, -0.5)) / 2560.0, (px[:, 1] + np.where(px[:, 1] >= 0, 0.5, -0.5)) / 1440.0], 1).astype(np.float32)
    back = np.stack([(xy[:, 0] * np.float32(2560)).astype(np.int32), (xy[:, 1] * np.float32(1440)).astype(np.int32)], 1)
    sel = (back == z['px']).all(1)
    assert sel.mean() > 0.99
    np.testing.assert_array_equal(tm.tilemap_px(z['px']), z['maps'])
    got = K.tilemap(torch.from_numpy(xy).cuda()).cpu().numpy().view(np.uint64)
    np.testing.assert_array_equal(got[sel], z['maps'][sel])
    assert len(np.unique(z['maps'])) > 400
    # the float path against the oracle on a wide random cloud (both truncate toward zero)
    rs = np.random.RandomState(8)
    cloud = (rs.rand(200000, 2) * 5.0 - 2.0).astype(np.float32)
    np.testing.assert_array_equal(K.tilemap(torch.from_numpy(cloud).cuda()).cpu().numpy().view(np.uint64), tm.tilemap_xy(cloud))
    for geom in ((1920, 1080, 6, 4, 400, 200), (2560, 1440, 32, 2, 90, 90)):
        np.testing.assert_array_equal(K.tilemap(torch.from_numpy(cloud).cuda(), *geom).cpu().numpy().view(np.uint64), tm.tilemap_xy(cloud, *geom))


def test_empty_and_degenerate_inputs(K):
    """Empty inputs are legal (the reference's loops simply do not run); degenerate 1x1x1 products and frame-edge pixels work."""
    d = 'cuda'
    assert K.tilemap(torch.zeros(0, 2, device=d)).shape == (0,)
    e = torch.zeros(0, dtype=torch.int64, device=d)
    assert K.tilemap_iou(e, e).shape == (0,) and K.tilemap_or_groups(e, 5).shape == (0,)
    assert K.gemm(torch.zeros(0, 64, device=d), torch.zeros(32, 64, device=d)).shape == (0, 32)
    assert K.gemm(torch.zeros(8, 64, device=d), torch.zeros(0, 64, device=d)).shape == (8, 0)
    np.testing.assert_array_equal(K.gemm(torch.full((1, 1), 3.0, device=d), torch.full((1, 1), 2.0, device=d)).cpu().numpy(), [[6.0]])
    from oracle import tilemap as otm
    xy = np.array([[0.0, 0.0], [1.0, 1.0], [0.99999994, 0.5], [0.5, 0.99999994], [0.1171875, 0.2083333]], np.float32)
    got = K.tilemap(torch.from_numpy(xy).to(d)).cpu().numpy().view(np.uint64)
    np.testing.assert_array_equal(got, otm.tilemap_xy(xy).view(np.uint64))


def test_find_tiles_covered_by_viewport_integer_pixel_edges():
    """The drop-in integer-pixel entry point (viewport_prediction/utils/common.py:46-58) on the frame edges and tile multiples --
    x in {0, 1, 319, 320, 321, 2559, 2560 = W, ...}, y in {0, 1, 179, 180, 181, 1439, 1440 = H, ...} -- against the imported
    reference function's maps (tests/golden/tilemap_px.npz): the wrapper turns the integer pixel into (x + 0.5) / W for the
    kernel's truncation, which must give the pixel back at both ends of the range."""
    from mansy_immersivevideostreaming_amd.viewport_prediction.utils.common import find_tiles_covered_by_viewport
    z = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'tilemap_px.npz'))
    ex = {0, 1, 299, 300, 301, 319, 320, 321, 639, 640, 2259, 2260, 2261, 2559, 2560}
    ey = {0, 1, 149, 150, 151, 179, 180, 181, 1289, 1290, 1291, 1439, 1440}
    n = 0
    for (x, y), want in zip(z['px'], z['maps']):
        if int(x) not in ex and int(y) not in ey:
            continue
        if int(x) not in ex and n % 3:          # thin the pure-y-edge rows: one launch per call
            n += 1
            continue
        n += 1
        m = find_tiles_covered_by_viewport(int(x), int(y), 2560, 1440, 320, 180, 8, 8)
        got = sum(int(b) << k for k, b in enumerate(m.reshape(-1)))
        assert got == int(want), (int(x), int(y), hex(got), hex(int(want)))
    assert n > 1000
    zo = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'tilemap_px_outside.npz'))      # centres outside the frame, negative pixels included
    for k in range(0, len(zo['px']), 97):
        x, y = (int(v) for v in zo['px'][k])
        m = find_tiles_covered_by_viewport(x, y, 2560, 1440, 320, 180, 8, 8)
        assert sum(int(b) << i for i, b in enumerate(m.reshape(-1))) == int(zo['maps'][k]), (x, y)
    for x, y in ((0, 0), (2560, 1440), (2560, 0), (0, 1440), (320, 180), (640, 180), (2560, 180)):     # corners / tile multiples are in the fixture
        assert ((z['px'][:, 0] == x) & (z['px'][:, 1] == y)).any(), (x, y)
