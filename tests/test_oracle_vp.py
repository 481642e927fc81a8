"""Pins oracle/vp_oracle.py (the CPU restatement) against golden vectors produced by the
IMPORTED reference (tools/gen_golden_vp.py): eval forward, sample(), train forward with both
MTIO branches, loss, full gradients, BN running stats and one AdamW step."""
import glob
import os
import numpy as np
import _golden
import pytest
import torch

from oracle import vp_oracle as vo

GOLD = sorted(p for p in glob.glob(os.path.join(os.path.dirname(__file__), 'golden', 'vp_*.npz')) if 'vp_loop_' not in os.path.basename(p))


def _load(path):
    z = _golden.load(path, allow_pickle=False)
    sd = vo.make_state_dict(int(z['d']), int(z['wseed']), bias=bool(z['bias']))
    return z, sd


@pytest.mark.parametrize('path', GOLD, ids=[os.path.basename(p)[:-4] for p in GOLD])
def test_eval_and_sample(path):
    z, sd = _load(path)
    orc = vo.VPOracle(sd, fut_window=int(z['T']))
    h, c = torch.from_numpy(z['history']), torch.from_numpy(z['current'])
    with torch.no_grad():
        pred = orc.process_src_current(torch.cat([h] * 3, -1), torch.cat([c] * 3, -1), train=False)
        samp = orc.sample(h, c)
    # fp32, tolerance from north_star: 1e-4 (observed ~1e-6)
    np.testing.assert_allclose(pred.numpy(), z['eval_pred'], atol=2e-5, rtol=0)
    np.testing.assert_allclose(samp.numpy(), z['eval_sample'], atol=2e-5, rtol=0)


@pytest.mark.parametrize('branch', ['rep', 'mix'])
@pytest.mark.parametrize('path', GOLD, ids=[os.path.basename(p)[:-4] for p in GOLD])
def test_train_forward_backward_adamw(path, branch):
    z, sd = _load(path)
    T = int(z['T'])
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items()
              if v.dtype.is_floating_point and 'running_' not in k and k != 'positional_embedding.pe'}
    full = dict(sd)
    full.update(params)
    orc = vo.VPOracle(full, fut_window=T)
    h, c, f = (torch.from_numpy(z[k]) for k in ('history', 'current', 'future'))
    perms = z[f'train_{branch}_perms']
    src, cur, gt = vo.mtio_mix(h, c, f, 3, repeat=(branch == 'rep'), perms=perms)
    np.testing.assert_array_equal(gt.numpy(), z[f'train_{branch}_gt'])
    pred = orc.process_src_current(src, cur, train=True)
    loss = orc.loss_function(pred, gt)
    loss.backward()
    np.testing.assert_allclose(pred.detach().numpy(), z[f'train_{branch}_pred'], atol=2e-5, rtol=0)
    np.testing.assert_allclose(loss.item(), float(z[f'train_{branch}_loss']), atol=1e-6, rtol=1e-5)
    names = [str(s) for s in z[f'train_{branch}_gradnames']]
    norms = z[f'train_{branch}_gradnorms']
    assert sorted(params) == names
    for k, n in zip(names, norms):
        g = params[k].grad
        assert g is not None, k
        # two fp32 CPU implementations (torch's fused modules vs explicit matmuls): 1e-4 on the synthetic B <= 8 cases, up to 1.1e-4
        # on the B = 32 real-trace batch (a bias gradient summed over 320 rows in a different order)
        assert abs(g.norm().item() - n) <= 3e-4 * max(n, 1e-3) + 1e-7, (k, g.norm().item(), n)
    for key in z.files:
        if key.startswith(f'train_{branch}_grad::'):
            k = key.split('::')[1]
            ref = z[key]
            tol = 1e-4 * np.abs(ref).max() + 1e-6  # conv bias grad is ~0 under train BN
            np.testing.assert_allclose(params[k].grad.numpy(), ref, atol=tol, rtol=0, err_msg=k)
        if key.startswith(f'train_{branch}_gradslice::'):
            k = key.split('::')[1]
            g = params[k].grad
            ref = z[key]
            tol = 1e-4 * np.abs(ref).max() + 1e-6  # conv bias grad is ~0 under train BN
            np.testing.assert_allclose(g.reshape(g.shape[0], -1)[::37, ::41].numpy(), ref, atol=tol, rtol=0)
    bn_mean, bn_var = orc.last_bn_stats
    np.testing.assert_allclose(bn_mean.numpy(), z[f'train_{branch}_bn_mean'], atol=1e-6, rtol=1e-5)
    np.testing.assert_allclose(bn_var.numpy(), z[f'train_{branch}_bn_var'], atol=1e-6, rtol=1e-5)
    for key in z.files:
        if key.startswith(f'train_{branch}_adamw::'):
            k = key.split('::')[1]
            p, g = params[k].detach(), params[k].grad
            gref = torch.from_numpy(z[f'train_{branch}_grad::{k}'])
            # the AdamW arithmetic on every element, from the reference's own gradient
            p1, _, _ = vo.adamw_step(p, gref, torch.zeros_like(p), torch.zeros_like(p), step=1)
            np.testing.assert_allclose(p1.numpy(), z[key], atol=2e-7, rtol=1e-6, err_msg=k)
            # from the oracle's gradient, on every element whose gradient the check above resolves: the first step moves a weight by
            # lr * g / (|g| + eps), so below the gradient tolerance the step follows the rounding of the CPU's matmul kernels, not the model
            p1, _, _ = vo.adamw_step(p, g, torch.zeros_like(p), torch.zeros_like(p), step=1)
            live = np.abs(z[f'train_{branch}_grad::{k}']) > 1e-4 * np.abs(z[f'train_{branch}_grad::{k}']).max() + 1e-6
            assert live.mean() > 0.5, (k, live.mean())
            np.testing.assert_allclose(p1.numpy()[live], z[key][live], atol=2e-7, rtol=1e-6, err_msg=k)


LOOPS = sorted(glob.glob(os.path.join(os.path.dirname(__file__), 'golden', 'vp_loop_*.npz')))


@pytest.mark.parametrize('path', LOOPS, ids=[os.path.basename(p)[:-4] for p in LOOPS])
def test_training_loop_vs_reference_capture(path):
    """The oracle through four consecutive iterations of run_models.py:37-44 + the validation metric (:50-58) against the capture
    of the imported reference (tools/gen_golden_vp_loop.py): MTIO decisions from the same host RNG stream (random.random(), then
    two np.random.shuffle per shuffled step -- mtio.py:77-87), AdamW moments and BatchNorm running statistics carried over."""
    import random
    z = _golden.load(path)
    d, T, B = int(z['d']), int(z['T']), int(z['B'])
    sd = vo.make_state_dict(d, int(z['wseed']), bias=bool(z['bias']))
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items()
              if v.dtype.is_floating_point and 'running_' not in k and k != 'positional_embedding.pe'}
    full = dict(sd)
    full.update(params)
    m = {k: torch.zeros_like(v) for k, v in params.items()}
    v2 = {k: torch.zeros_like(v) for k, v in params.items()}
    seed, lr = int(z['seed']), float(z['lr'])
    np.random.seed(seed); torch.manual_seed(seed); random.seed(seed)
    losses = []
    for i in range(len(z['losses'])):
        h, c, f = (torch.from_numpy(z[f'b{i}/{k}']) for k in ('history', 'current', 'future'))
        repeat = random.random() < 0.5
        assert repeat == bool(z['repeat'][i])
        perms = None
        if not repeat:
            perms = []
            for _ in range(2):
                idx = np.arange(B)
                np.random.shuffle(idx)
                perms.append(idx.copy())
        src, cur, gt = vo.mtio_mix(h, c, f, 3, repeat, perms)
        orc = vo.VPOracle(full, fut_window=T)
        loss = orc.loss_function(orc.process_src_current(src, cur, train=True), gt)
        for p in params.values():
            p.grad = None
        loss.backward()
        losses.append(loss.item())
        bn_mean, bn_var = orc.last_bn_stats
        full['transformer.distill_layer.norm.running_mean'], full['transformer.distill_layer.norm.running_var'] = bn_mean, bn_var
        with torch.no_grad():
            for k, p in params.items():
                p1, m[k], v2[k] = vo.adamw_step(p, p.grad, m[k], v2[k], step=i + 1, lr=lr)
                p.copy_(p1)
    np.testing.assert_allclose(losses, z['losses'], rtol=2e-4, atol=2e-6)
    bn = 'final::transformer.distill_layer.norm.'
    # (tolerances: see tests/test_gpu_vp_engine.py::test_training_loop_vs_reference_capture -- zero-gradient parameters random-walk)
    np.testing.assert_allclose(full['transformer.distill_layer.norm.running_mean'].numpy(), z[bn + 'running_mean'], atol=6e-4, rtol=0)
    np.testing.assert_allclose(full['transformer.distill_layer.norm.running_var'].numpy(), z[bn + 'running_var'], atol=6e-4, rtol=1e-3)
    for k, p in params.items():
        err = np.abs(p.detach().numpy() - z['final::' + k])
        noise_driven = k.endswith('downConv.bias') or k.endswith('in_proj_bias') or k.endswith('transformer.encoder.norm.bias')
        assert (noise_driven or float((err > 4e-5).mean()) <= 0.02) and err.max() <= 8.5e-4, (k, float((err > 4e-5).mean()), float(err.max()))
    with torch.no_grad():
        orc = vo.VPOracle({k: (v.detach() if torch.is_tensor(v) else v) for k, v in full.items()}, fut_window=T)
        mse = []
        for i in range(2):
            h, c, f = (torch.from_numpy(z[f'v{i}/{k}']) for k in ('history', 'current', 'future'))
            pred = orc.sample(h, c)
            e = torch.abs(pred - f)
            e = torch.minimum(e, torch.abs(pred + 1 - f))
            e = torch.minimum(e, torch.abs(pred - 1 - f))
            mse.append(torch.mean(torch.sum(e * e, dim=-1) / 2).item())
    np.testing.assert_allclose(np.sum(mse) / 2, float(z['valid_mse']), rtol=2e-3, atol=1e-6)


@pytest.mark.parametrize('tag,T', [('s5_t15', 15), ('s10_t10', 10), ('syn', 12)])
def test_linear_regression_baseline_vs_imported_reference(tag, T):
    """oracle.linear_regression_sample against the imported reference class (scikit-learn per trajectory; tools/gen_golden_linreg.py):
    bit-equal on the real Jin2022 windows; on the synthetic stress rows the closed form and LAPACK's least squares may differ in
    the last float64 bits, which survives the rounding to float32 for under 1 % of the values, by one ulp."""
    z = _golden.load(os.path.join(os.path.dirname(__file__), 'golden', 'linreg_reference.npz'))
    got = vo.linear_regression_sample(z[f'{tag}_history'], z[f'{tag}_current'], T)
    want = z[f'{tag}_pred']
    assert got.dtype == np.float32 and got.shape == want.shape
    np.testing.assert_allclose(got, want, rtol=2e-7, atol=1e-7)
    assert (got == want).mean() > 0.99
    if tag != 'syn':
        np.testing.assert_array_equal(got, want)
