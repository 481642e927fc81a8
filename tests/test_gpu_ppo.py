"""GPU parity of the bitrate-selection networks and PPO machinery (libmansy_hip.so through the drop-in classes):
  * FeatureNet/Actor/Critic/QoEIdentifier outputs, identifier reward and a full train_identifier() call against golden
    vectors of the imported reference (tests/golden/ppo_reference.npz);
  * Categorical sampling: bit-exact actions vs the oracle's inverse-CDF sampler on the same uniforms;
  * PPO minibatch loss/gradients/clip/Adam, GAE + running return normaliser against oracle/ppo_oracle.py
    (tianshou-0.4.8 restatement: parity UNPINNED, see that file);
  * an end-to-end collect -> train_identifier -> relabel -> update cycle on synthetic bench-shaped tables."""
import ctypes
import os

import numpy as np
import _golden
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ppo_oracle as po  # noqa: E402

Z = _golden.load(os.path.join(os.path.dirname(__file__), 'golden', 'ppo_reference.npz'))


@pytest.fixture(scope='module')
def M():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a ROCm device (no CPU fallback exists)')
    from mansy_immersivevideostreaming_amd.bitrate_selection.models import mansy, mansy_ppo
    from mansy_immersivevideostreaming_amd.bitrate_selection.envs import mansy_env

    class NS:
        pass
    ns = NS()
    ns.mansy, ns.ppo, ns.env = mansy, mansy_ppo, mansy_env
    return ns


class Args:
    use_identifier = True
    lamb = 0.5


def build_policy(M, sd, lr=5e-4, ilr=1e-4, wd=1e-2, **policy_kw):
    mm = M.mansy
    fn = mm.FeatureNet(8, 64, 5, 128, device='cuda')
    actor = mm.Actor(fn, 1280, 128, 15, 'cuda')
    critic = mm.Critic(fn, 1280, 128, 'cuda')
    ifn = mm.QoEIdentifierFeatureNet(8, 64, 5, 15, 128, device='cuda')
    ident = mm.QoEIdentifier(ifn, 1280, 128, 'cuda')
    optim = torch.optim.Adam(list(actor.parameters()) + [p for n, p in critic.named_parameters() if not n.startswith('feature_net.')], lr=lr,
                             weight_decay=wd)
    ioptim = torch.optim.Adam(ident.parameters(), lr=ilr, weight_decay=wd)
    kw = dict(discount_factor=0.95, max_grad_norm=1.0, eps_clip=0.2, vf_coef=0.5, ent_coef=0.02, reward_normalization=1, advantage_normalization=1,
              value_clip=1, gae_lambda=0.95, action_space=15, args=Args(), identifier=ident, identifier_optim=ioptim)
    kw.update(policy_kw)
    pol = M.ppo.PPOPolicy(actor, critic, optim, lambda lg: torch.distributions.Categorical(logits=lg), **kw)
    pol.load_state_dict(sd)
    return pol.to('cuda')


def test_state_dict_layout_and_forward_vs_reference(M):
    sd = po.make_policy_state_dict(int(Z['wseed']))
    pol = build_policy(M, sd)
    assert list(pol.state_dict().keys()) == list(sd.keys())            # 120 keys, shipped checkpoint order
    for k, v in pol.state_dict().items():
        assert torch.equal(v.cpu(), sd[k]), k
    obs = torch.from_numpy(Z['obs'][:64]).cuda()
    logits, _ = pol.actor(obs)
    value = pol.critic(obs)
    pred = pol.identifier(obs)
    np.testing.assert_allclose(logits.cpu().numpy(), Z['logits'], atol=2e-5, rtol=1e-5)
    np.testing.assert_allclose(value.cpu().numpy(), Z['value'], atol=2e-5, rtol=1e-5)
    np.testing.assert_allclose(pred.cpu().numpy(), Z['ident'], atol=2e-6, rtol=1e-5)
    assert (logits.argmax(-1).cpu().numpy() == Z['logits'].argmax(-1)).all()         # bitrate decisions identical
    # the reference's dict-of-numpy observation form (tianshou Batch style)
    from mansy_immersivevideostreaming_amd.bitrate_selection.envs.mansy_env import OBS_SLICES
    rows = Z['obs'][:64]
    d = {k: rows[:, a:b].reshape((64,) + shape) for k, (a, b, shape) in OBS_SLICES.items()}
    logits2, _ = pol.actor(d)
    assert torch.equal(logits, logits2)
    pred2 = pol.identifier(d, d['action_one_hot'])
    assert torch.equal(pred, pred2)


def test_identifier_reward_and_relabel(M):
    sd = po.make_policy_state_dict(int(Z['wseed']))
    pol = build_policy(M, sd)
    rows = Z['ident_reward_rows']
    buf = M.ppo.RolloutBuffer(len(rows), 1, 'cuda')
    buf.obs[:, 0] = torch.from_numpy(Z['obs'][rows]).cuda()
    buf.rew[:, 0] = 0.25
    buf.filled = len(rows)
    pol.relabel(buf, lamb=0.5)
    want = 0.5 * 0.25 + 0.5 * Z['ident_reward']
    np.testing.assert_allclose(buf.rew[:, 0].cpu().numpy(), want, atol=1e-6, rtol=0)


def test_train_identifier_vs_reference(M):
    sd = po.make_policy_state_dict(int(Z['wseed']))
    pol = build_policy(M, sd)
    n = int(Z['ti_n'])
    buf = M.ppo.RolloutBuffer(n, 1, 'cuda')
    buf.obs[:, 0] = torch.from_numpy(Z['obs'][:n]).cuda()
    buf.filled = n
    np.random.seed(int(Z['ti_npseed']))
    losses, vloss = pol.train_identifier(buf, update_round=2, verbose=False)
    got = [l.item() for l in losses] + [vloss.item()]
    np.testing.assert_allclose(got, Z['ti_losses'], rtol=5e-5, atol=1e-7)
    after = pol.state_dict()
    for key in Z.files:
        if key.startswith('ti_after::'):
            np.testing.assert_allclose(after[key[10:]].cpu().numpy(), Z[key], atol=3e-6, rtol=1e-5, err_msg=key)


def test_categorical_sampling_bit_exact_decisions(M):
    sd = po.make_policy_state_dict(int(Z['wseed']))
    pol = build_policy(M, sd)
    obs = torch.from_numpy(Z['obs'][:250]).cuda()
    u = torch.rand(250, generator=torch.Generator().manual_seed(4))
    logits, _, act, logp = pol.engine.policy_forward(obs, want_value=False, sample=True, u=u.cuda())
    want = po.categorical_sample(logits.cpu(), u)
    assert (act.cpu().long() == want).all()
    lp = torch.log_softmax(logits.cpu().double(), -1).gather(1, want[:, None])[:, 0]
    np.testing.assert_allclose(logp.cpu().numpy(), lp.numpy(), atol=2e-6)
    # hash-driven sampling: deterministic given (seed, site) and distributed like the softmax
    _, _, a1, _ = pol.engine.policy_forward(obs, want_value=False, sample=True, seed=7, site=3)
    _, _, a2, _ = pol.engine.policy_forward(obs, want_value=False, sample=True, seed=7, site=3)
    assert torch.equal(a1, a2)


def _minibatch_data(n=96):
    g = torch.Generator().manual_seed(9)
    obs = torch.from_numpy(Z['obs'][:n])
    act = torch.randint(0, 15, (n,), generator=g)
    adv = torch.randn(n, generator=g)
    v_old = torch.randn(n, generator=g) * 0.3
    ret = torch.randn(n, generator=g) * 0.5
    return obs, act, adv, v_old, ret, g


def _oracle_grads(sd, obs, act, adv, logp_old, v_old, ret, **loss_kw):
    uniq, params = {}, {}
    for k, v in sd.items():
        if k.startswith('_actor_critic.') or k.startswith('identifier.'):
            continue
        key = k.replace('critic.feature_net.', 'actor.feature_net.')
        if key not in uniq:
            uniq[key] = v.clone().requires_grad_(True)
        params[k] = uniq[key]
    loss, clip, vf, ent = po.ppo_loss(po.actor_logits(params, obs), po.critic_value(params, obs), act, adv, logp_old, v_old, ret, **loss_kw)
    loss.backward()
    return uniq, (loss.item(), clip.item(), vf.item(), ent.item())


def test_ppo_minibatch_loss_grads_clip_adam_vs_oracle(M):
    sd = po.make_policy_state_dict(int(Z['wseed']))
    pol = build_policy(M, sd)
    obs, act, adv, v_old, ret, g = _minibatch_data()
    with torch.no_grad():
        logp_old = torch.log_softmax(po.actor_logits(sd, obs), -1).gather(1, act[:, None])[:, 0] + 0.3 * torch.randn(len(obs), generator=g)
    uniq, (loss, clip, vf, ent) = _oracle_grads(sd, obs, act, adv, logp_old, v_old, ret)
    from mansy_immersivevideostreaming_amd._lib import check, lib, ptr, stream_ptr
    eng, f = pol.engine, pol.engine.ac
    dev = 'cuda'
    d = dict(obs=obs.to(dev), act=act.int().to(dev), adv=adv.to(dev), logp=logp_old.to(dev), v=v_old.to(dev), ret=ret.to(dev))
    stats = torch.zeros(4, device=dev)

    def call(step, max_norm):
        arr, garr = f.pointers(grads=True)
        check(lib().mansy_ppo_minibatch_step(arr, garr, ptr(f.flat_p), ptr(f.flat_g), ptr(f.m), ptr(f.v), f.flat_p.numel(), ptr(d['obs']), None,
                                             ptr(d['act']), ptr(d['adv']), ptr(d['logp']), ptr(d['v']), ptr(d['ret']), len(obs), 0.2, 0.5, 0.02, 1, 1, 0.0,
                                             max_norm, 5e-4, 1e-2, step, -1, 0, ptr(stats), ptr(eng.workspace()), eng.max_batch, 0, None, 0, None, None, eng.prec, stream_ptr()), 'ppo_mb')
    call(0, 0.0)                                  # gradients only, no clipping
    np.testing.assert_allclose(stats.cpu().numpy(), [loss, clip, vf, ent], rtol=2e-5, atol=2e-6)
    names = [n for n, _ in f.table]
    gnorm2 = 0.0
    for n_, o, p in zip(names, f.offsets, f.params):
        got = f.flat_g[o:o + p.numel()].view(p.shape).cpu().numpy()
        ref = uniq[n_].grad.numpy()
        gnorm2 += float((ref.astype(np.float64) ** 2).sum())
        np.testing.assert_allclose(got, ref, atol=3e-5 * max(np.abs(ref).max(), 1e-3), rtol=0, err_msg=n_)
    # clipped + Adam(L2): compare first-moment buffers (linear in the clipped gradient + wd * p)
    max_norm = 0.5 * gnorm2 ** 0.5
    call(1, max_norm)
    coef = max_norm / (gnorm2 ** 0.5 + 1e-6)
    for n_, o, p in zip(names, f.offsets, f.params):
        m = f.m[o:o + p.numel()].view(p.shape).cpu().numpy()
        ref = 0.1 * (coef * uniq[n_].grad.numpy() + 1e-2 * sd[n_].numpy())
        np.testing.assert_allclose(m, ref, atol=3e-5 * max(np.abs(ref).max(), 1e-4), rtol=0, err_msg=n_)
    # parameters moved by at most lr (Adam step 1) and in the direction of -m
    k = names.index('actor.fc.0.weight')
    o, p = f.offsets[k], f.params[k]
    delta = (p.detach().cpu() - sd['actor.fc.0.weight']).numpy()
    assert np.abs(delta).max() <= 5e-4 * 1.001
    mm_ = f.m[o:o + p.numel()].view(p.shape).cpu().numpy()
    big = np.abs(mm_) > 1e-6
    assert (np.sign(delta[big]) == -np.sign(mm_[big])).all()


def test_paired_launch_of_the_fc_weight_gradients_and_dF_is_bit_identical_to_two_launches(M):
    """Round 4: the minibatch step's fc weight-gradient pair and its dF product are independent readers of dA1 and run as ONE launch
    (gemm_f32_wsk_dual_kernel: the same two loop bodies on disjoint workgroup ranges of one grid).  ABI 8: the release library has no switch
    for it; the -DMANSY_LAB build of the same sources has (default variant 0x800 = no paired launch).  Every gradient, the loss statistics and
    the identifier's training step (fc_bwd_single's pair) are bit-identical either way -- and the release library agrees with both."""
    import sys
    from mansy_immersivevideostreaming_amd import _lib as LB, build_ext
    from mansy_immersivevideostreaming_amd._lib import check, ptr, stream_ptr
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import lab_knobs                  # the lab-library harness lives with the tools (the package holds no swappable library handle)
    build_ext.build(lab=True)
    sd = po.make_policy_state_dict(int(Z['wseed']))
    obs, act, adv, v_old, ret, g = _minibatch_data()
    logp_old = torch.log_softmax(po.actor_logits(sd, obs), -1).gather(1, act[:, None])[:, 0] + 0.3 * torch.randn(len(obs), generator=g)
    dev = 'cuda'
    d = dict(obs=obs.to(dev), act=act.int().to(dev), adv=adv.to(dev), logp=logp_old.to(dev), v=v_old.to(dev), ret=ret.to(dev))
    outs = {}

    def run(L):
        pol = build_policy(M, sd)
        eng, f, fi = pol.engine, pol.engine.ac, pol.engine.idn
        stats = torch.zeros(4, device=dev)
        arr, garr = f.pointers(grads=True)
        check(L.mansy_ppo_minibatch_step(arr, garr, ptr(f.flat_p), ptr(f.flat_g), ptr(f.m), ptr(f.v), f.flat_p.numel(), ptr(d['obs']), None,
                                         ptr(d['act']), ptr(d['adv']), ptr(d['logp']), ptr(d['v']), ptr(d['ret']), len(obs), 0.2, 0.5, 0.02, 1, 1, 0.0,
                                         0.0, 5e-4, 1e-2, 0, -1, 0, ptr(stats), ptr(eng.workspace()), eng.max_batch, 0, None, 0, None, None, eng.prec, stream_ptr()), 'ppo_mb')
        iloss = torch.zeros((), device=dev)
        iarr, igarr = fi.pointers(grads=True)
        check(L.mansy_identifier_train_step(iarr, igarr, ptr(fi.flat_p), ptr(fi.flat_g), ptr(fi.m), ptr(fi.v), fi.flat_p.numel(), ptr(d['obs']), None,
                                            len(obs), 1e-4, 1e-2, -1, ptr(iloss), ptr(eng.workspace()), eng.max_batch, None, None, eng.prec, stream_ptr()), 'ident')
        torch.cuda.synchronize()
        return (f.flat_g.clone(), stats.clone(), fi.flat_g.clone(), iloss.clone())
    for knob, variant in ((8, 0x800), (9, 0)):
        with lab_knobs.lab_library(variant) as L:
            outs[knob] = run(L)
    rel = run(LB.lib())
    for a, b in zip(rel, outs[9]):
        assert torch.equal(a, b)
    assert float(outs[9][0].abs().max()) > 0 and float(outs[9][2].abs().max()) > 0
    for a, b in zip(outs[8][:2], outs[9][:2]):
        assert torch.equal(a, b)
    # the identifier's dbbd / fc bias row sums are float atomics on the 64 x 64 loop for batches of this size: compare to rounding there
    assert torch.equal(outs[8][3], outs[9][3])
    assert (outs[8][2] - outs[9][2]).abs().max().item() <= 1e-6 * float(outs[9][2].abs().max())


@pytest.mark.parametrize('flags', [dict(dual_clip=3.0), dict(dual_clip=1.5, value_clip=False), dict(norm_adv=False, dual_clip=2.0),
                                   dict(norm_adv=False, value_clip=False)])
def test_ppo_minibatch_flag_combinations_incl_dual_clip_vs_oracle(M, flags):
    """The PPO flags of the reference's command line that its defaults leave off (run_mansy.py --dual-clip / --value-clip 0 / --norm-adv 0):
    loss terms and every gradient of one minibatch step against the oracle's autograd.  Policy ratios are pushed far from 1 (log-prob
    offsets up to +-2) so that, with negative advantages, the dual-clip bound max(min(surr1, surr2), c * adv) is the active branch for a
    good part of the rows (T2: tianshou ppo.py)."""
    sd = po.make_policy_state_dict(int(Z['wseed']))
    pol = build_policy(M, sd)
    obs, act, adv, v_old, ret, g = _minibatch_data()
    with torch.no_grad():
        logp_old = torch.log_softmax(po.actor_logits(sd, obs), -1).gather(1, act[:, None])[:, 0] + 1.0 * torch.randn(len(obs), generator=g)
    okw = dict(norm_adv=flags.get('norm_adv', True), value_clip=flags.get('value_clip', True), dual_clip=flags.get('dual_clip'))
    uniq, (loss, clip, vf, ent) = _oracle_grads(sd, obs, act, adv, logp_old, v_old, ret, **okw)
    if okw['dual_clip']:            # the bound really is active somewhere: the loss differs from the plain clipped surrogate's
        _, (_, clip_plain, _, _) = _oracle_grads(sd, obs, act, adv, logp_old, v_old, ret, norm_adv=okw['norm_adv'], value_clip=okw['value_clip'])
        assert abs(clip_plain - clip) > 1e-3
    from mansy_immersivevideostreaming_amd._lib import check, lib, ptr, stream_ptr
    eng, f = pol.engine, pol.engine.ac
    d = dict(obs=obs.cuda(), act=act.int().cuda(), adv=adv.cuda(), logp=logp_old.cuda(), v=v_old.cuda(), ret=ret.cuda())
    stats = torch.zeros(4, device='cuda')
    arr, garr = f.pointers(grads=True)
    check(lib().mansy_ppo_minibatch_step(arr, garr, ptr(f.flat_p), ptr(f.flat_g), ptr(f.m), ptr(f.v), f.flat_p.numel(), ptr(d['obs']), None,
                                         ptr(d['act']), ptr(d['adv']), ptr(d['logp']), ptr(d['v']), ptr(d['ret']), len(obs), 0.2, 0.5, 0.02,
                                         int(okw['norm_adv']), int(okw['value_clip']), float(okw['dual_clip'] or 0.0), 0.0, 5e-4, 1e-2, 0, -1, 0,
                                         ptr(stats), ptr(eng.workspace()), eng.max_batch, 0, None, 0, None, None, eng.prec, stream_ptr()), 'ppo_mb')
    np.testing.assert_allclose(stats.cpu().numpy(), [loss, clip, vf, ent], rtol=2e-5, atol=2e-6)
    for n_, o, p in zip([n for n, _ in f.table], f.offsets, f.params):
        got = f.flat_g[o:o + p.numel()].view(p.shape).cpu().numpy()
        ref = uniq[n_].grad.numpy()
        np.testing.assert_allclose(got, ref, atol=3e-5 * max(np.abs(ref).max(), 1e-3), rtol=0, err_msg=n_)
    with pytest.raises(Exception):            # tianshou asserts dual_clip > 1
        build_policy(M, sd, dual_clip=0.9)


def test_update_with_recompute_advantage_and_dual_clip_vs_oracle(M):
    """PPOPolicy(recompute_advantage=True, dual_clip=2.0).update against the oracle's restatement of tianshou's learn loop: before the
    second pass the CURRENT critic's values, GAE, returns and the running return statistics are redone (ret_rms absorbs the buffer twice
    per update: its count pins that the recompute happened), logp_old is kept.  First pass tight; the rows after the recompute start from
    weights eight Adam steps in, so they carry the same value-clip boundary caveat as test_whole_update_vs_oracle_update."""
    sd = po.make_policy_state_dict(int(Z['wseed']))
    T, N, bs = 16, 256, 512
    pol = build_policy(M, sd, recompute_advantage=True, dual_clip=2.0)
    rs = np.random.RandomState(4)
    n = T * N
    src = Z['obs']
    obs = src[rs.randint(0, len(src), size=n)].reshape(T, N, 780).copy()
    obs_next = src[rs.randint(0, len(src), size=n)].reshape(T, N, 780).copy()
    act = rs.randint(0, 15, size=(T, N)).astype(np.int32)
    rew = rs.randn(T, N).astype(np.float32)
    done = rs.rand(T, N) < 0.05
    buf = M.ppo.RolloutBuffer(T, N, 'cuda')
    buf.obs.copy_(torch.from_numpy(obs)); buf.obs_next.copy_(torch.from_numpy(obs_next)); buf.act.copy_(torch.from_numpy(act))
    buf.rew.copy_(torch.from_numpy(rew)); buf.done.copy_(torch.from_numpy(done.astype(np.uint8)))
    buf.filled = T
    np.random.seed(7)
    res = pol.update(0, buf, is_train=True, batch_size=bs, repeat=2)
    got_rows = np.stack([res['loss'], res['loss/clip'], res['loss/vf'], res['loss/ent']], 1)
    np.random.seed(7)
    rms_o, ost = po.RunningMeanStd(), {}
    want_rows, inter = po.update({k: v.clone() for k, v in sd.items()}, obs, obs_next, act, rew, done, rms_o, ost, lamb=0.5, batch_size=bs, repeat=2,
                                 dual_clip=2.0, recompute_adv=True)
    assert got_rows.shape == want_rows.shape == (16, 4)
    assert rms_o.count == 2 * n
    np.testing.assert_allclose(pol.ret_rms().cpu().numpy(), [rms_o.mean, rms_o.var, rms_o.count], rtol=2e-3)
    np.testing.assert_allclose(got_rows[:2], want_rows[:2], rtol=1e-5, atol=3e-6)
    np.testing.assert_allclose(got_rows[:8], want_rows[:8], rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(got_rows, want_rows, rtol=3e-2, atol=2e-3)
    # the recompute changes the second pass: without it the rows 8.. differ visibly (same seed, same data)
    pol2 = build_policy(M, sd, dual_clip=2.0)
    buf.rew.copy_(torch.from_numpy(rew))
    np.random.seed(7)
    res2 = pol2.update(0, buf, is_train=True, batch_size=bs, repeat=2)
    assert abs(np.asarray(res2['loss/vf'])[8] - got_rows[8, 2]) > 1e-4 * abs(got_rows[8, 2])
    np.testing.assert_allclose(np.asarray(res2['loss'])[:8], got_rows[:8, 0], rtol=1e-5, atol=1e-6)
    assert float(pol2.ret_rms().cpu().numpy()[2]) == n


@pytest.mark.parametrize('T,N', [(16, 40), (16, 256), (3, 1100)])       # N <= 1024: the single-launch form; above: four launches
def test_gae_and_return_normaliser_vs_oracle(M, T, N):
    from mansy_immersivevideostreaming_amd._lib import check, lib, ptr, stream_ptr
    rs = np.random.RandomState(2)
    rms_o = po.RunningMeanStd()
    rms_d = torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64, device='cuda')
    for it in range(3):
        rew = rs.randn(T, N).astype(np.float32)
        v_s = rs.randn(T, N).astype(np.float32)
        v_n = rs.randn(T, N).astype(np.float32)
        done = (rs.rand(T, N) < 0.1)
        want_ret = np.zeros((T, N), np.float32)
        want_adv = np.zeros((T, N), np.float32)
        # oracle: tianshou processes the whole buffer at once -> returns of all envs normalised with the same old variance
        scale = np.sqrt(rms_o.var + 1e-8)
        unn = []
        for e in range(N):
            end = done[:, e].copy()
            end[-1] = True
            r_un, adv = po.gae_returns(rew[:, e], v_s[:, e].astype(np.float64) * scale, v_n[:, e].astype(np.float64) * scale, done[:, e], end, 0.95, 0.95)
            want_adv[:, e] = adv
            want_ret[:, e] = r_un / scale
            unn.append(r_un)
        rms_o.update(np.concatenate(unn))
        ret = torch.empty(T * N, device='cuda')
        adv = torch.empty(T * N, device='cuda')
        scratch = torch.empty(T * N + 2, dtype=torch.float64, device='cuda')
        keep = [torch.from_numpy(rew).cuda(), torch.from_numpy(v_s).cuda(), torch.from_numpy(v_n).cuda(),
                torch.from_numpy(done.astype(np.uint8)).cuda()]          # keep the device inputs alive across the async call
        check(lib().mansy_gae_returns(ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), ptr(keep[3]), T, N, 0.95, 0.95, 1, ptr(rms_d), ptr(scratch), ptr(ret),
                                      ptr(adv), stream_ptr()), 'gae')
        torch.cuda.synchronize()
        np.testing.assert_allclose(adv.cpu().numpy().reshape(T, N), want_adv, rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(ret.cpu().numpy().reshape(T, N), want_ret, rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(rms_d.cpu().numpy(), [rms_o.mean, rms_o.var, rms_o.count], rtol=1e-10)


def test_gae_kernel_reproduces_tianshou_published_known_answers(M):
    """P5 pin on the HIP path: mansy_gae_returns on the vectors tianshou's own repository publishes for compute_episodic_return
    (v0.4.8 test/base/test_returns.py; tests/golden/tianshou_known_answers.npz, tools/gen_golden_tianshou_ka.py -- TYPED IN from that published test, tianshou is
    not installable here: the vectors are authentic to the best of the builder's knowledge, they were not generated by running tianshou): one
    environment (N = 1), each case alone and all four side by side as the columns of one padded [T][N] launch."""
    from mansy_immersivevideostreaming_amd._lib import check, lib, ptr, stream_ptr
    KA = _golden.load(os.path.join(os.path.dirname(__file__), 'golden', 'tianshou_known_answers.npz'))
    for i in range(int(KA['n_cases'])):
        rew, v_s, v_n, done = (KA[f'c{i}_{k}'] for k in ('rew', 'v_s', 'v_next', 'done'))
        T = len(rew)
        keep = [torch.from_numpy(rew.astype(np.float32)).cuda(), torch.from_numpy(v_s.astype(np.float32)).cuda(),
                torch.from_numpy(v_n.astype(np.float32)).cuda(), torch.from_numpy(done.astype(np.uint8)).cuda()]
        ret, adv = torch.empty(T, device='cuda'), torch.empty(T, device='cuda')
        scratch = torch.empty(T + 2, dtype=torch.float64, device='cuda')
        rms = torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64, device='cuda')
        check(lib().mansy_gae_returns(ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), ptr(keep[3]), T, 1, float(KA[f'c{i}_gamma']),
                                      float(KA[f'c{i}_lambda']), 0, ptr(rms), ptr(scratch), ptr(ret), ptr(adv), stream_ptr()), 'gae')
        torch.cuda.synchronize()
        np.testing.assert_allclose(ret.cpu().numpy(), KA[f'c{i}_returns'], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(adv.cpu().numpy(), KA[f'c{i}_returns'] - v_s, rtol=1e-5, atol=1e-5)
        # with the return normaliser on and its initial state (var 1): returns / sqrt(1 + 1e-8), moments = those of the returns
        check(lib().mansy_gae_returns(ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), ptr(keep[3]), T, 1, float(KA[f'c{i}_gamma']),
                                      float(KA[f'c{i}_lambda']), 1, ptr(rms), ptr(scratch), ptr(ret), ptr(adv), stream_ptr()), 'gae')
        torch.cuda.synchronize()
        np.testing.assert_allclose(ret.cpu().numpy(), KA[f'c{i}_returns'], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(rms.cpu().numpy(), [KA[f'c{i}_returns'].mean(), KA[f'c{i}_returns'].var(), T], rtol=1e-5)


def _engine_load(f, uniq, m, v, step):
    """Teacher forcing: the oracle's unique weights and Adam moments into the engine's flat buffers."""
    for name, o, p in zip([t[0] for t in f.table], f.offsets, f.params):
        n = p.numel()
        f.flat_p[o:o + n].copy_(uniq[name].detach().reshape(-1))
        f.m[o:o + n].copy_(m[name].reshape(-1))
        f.v[o:o + n].copy_(v[name].reshape(-1))
    f.step = step


def test_update_teacher_forced_every_minibatch_step(M):
    """P6 pin that bites on ALL 16 (and the ragged 4) minibatch steps of two consecutive updates: before each step the oracle's
    weights and Adam moments are copied into the engine, ONE mansy_ppo_minibatch_step runs on the oracle's index set and the
    oracle's process_fn outputs, and the loss row and the post-step weights are compared -- no trajectory divergence can
    accumulate, so the second pass's re-permutation, merge_last on the ragged buffer, the per-minibatch advantage normalisation,
    the value clip, gradient clip and Adam(L2) are each checked at every step.  (The free-running comparison stays in
    test_whole_update_vs_oracle_update.)"""
    from mansy_immersivevideostreaming_amd._lib import check, lib, ptr, stream_ptr
    sd = po.make_policy_state_dict(int(Z['wseed']))
    lr, wd = 5e-4, 1e-2
    for (T, N, bs) in ((16, 256, 512), (11, 100, 512)):
        pol = build_policy(M, sd)
        eng, f = pol.engine, pol.engine.ac
        rs = np.random.RandomState(3)
        n = T * N
        src = Z['obs']
        obs = src[rs.randint(0, len(src), size=n)].reshape(T, N, 780).copy()
        obs_next = src[rs.randint(0, len(src), size=n)].reshape(T, N, 780).copy()
        act = rs.randint(0, 15, size=(T, N)).astype(np.int32)
        rew = rs.randn(T, N).astype(np.float32)
        done = rs.rand(T, N) < 0.05
        rms_o, ost = po.RunningMeanStd(), {}
        obs_d = torch.from_numpy(obs.reshape(n, 780)).cuda()
        act_d = torch.from_numpy(act.reshape(n)).cuda()
        for it in range(2):
            snaps, posts = [], []

            def before(k, idx, st, inter):
                snaps.append(dict(idx=idx.astype(np.int32).copy(), inter=inter,
                                  w={a: b.detach().clone() for a, b in st['uniq'].items()},
                                  m={a: b.clone() for a, b in st['m'].items()}, v={a: b.clone() for a, b in st['v'].items()},
                                  step=dict(st['step'])))

            def after(k, uniq):
                posts.append({a: b.detach().clone() for a, b in uniq.items()})
            np.random.seed(100 + it)
            sd_now = {k: v.clone() for k, v in sd.items()}
            rows, inter = po.update(sd_now, obs, obs_next, act, rew + 0.1 * it, done, rms_o, ost, lamb=0.5, batch_size=bs, repeat=2,
                                    on_step=after, before_step=before)
            assert len(snaps) == len(posts) == len(rows) == (16 if n == 4096 else 4)
            if n != 4096:
                assert sorted(len(s['idx']) for s in snaps) == [512, 512, 588, 588]          # merge_last on the ragged buffer
            data = {k: torch.from_numpy(np.ascontiguousarray(inter[k])).cuda() for k in ('adv', 'logp_old', 'v_s', 'returns')}
            worst = 0.0
            edge_steps = []
            for k, (sn, post) in enumerate(zip(snaps, posts)):
                steps = set(sn['step'].values())
                assert len(steps) == 1
                _engine_load(f, sn['w'], sn['m'], sn['v'], steps.pop() + 1)
                idx = torch.from_numpy(sn['idx']).cuda()
                stats = torch.empty(4, device='cuda')
                arr, garr = f.pointers(grads=True)
                check(lib().mansy_ppo_minibatch_step(arr, garr, ptr(f.flat_p), ptr(f.flat_g), ptr(f.m), ptr(f.v), f.flat_p.numel(), ptr(obs_d), ptr(idx),
                                                     ptr(act_d), ptr(data['adv']), ptr(data['logp_old']), ptr(data['v_s']), ptr(data['returns']),
                                                     idx.numel(), 0.2, 0.5, 0.02, 1, 1, 0.0, 1.0, lr, wd, f.step, *f.tail(), ptr(stats),
                                                     ptr(eng.workspace()), eng.max_batch, 0, None, 0, None, None, eng.prec, stream_ptr()), 'mansy_ppo_minibatch_step')
                torch.cuda.synchronize()
                np.testing.assert_allclose(stats.cpu().numpy(), rows[k], rtol=1e-5, atol=3e-6, err_msg=f'{(T, N, it, k)}')
                n_el = n_bad = 0
                per = {}
                for name, o, p in zip([t[0] for t in f.table], f.offsets, f.params):
                    got = f.flat_p[o:o + p.numel()].cpu().numpy()
                    want = post[name].numpy().reshape(-1)
                    err = np.abs(got - want)
                    # Adam's step is lr * m_hat / (sqrt(v_hat) + eps): where the gradient is at rounding-noise level and v_hat ~ 0
                    # (first steps) a sign flip is a whole lr; everywhere else the two steps agree to a small fraction of lr
                    assert err.max() <= 2.0 * lr * 1.001, (T, N, it, k, name, float(err.max()))
                    n_el += err.size
                    n_bad += int((err > 0.05 * lr).sum())
                    if (err > 0.05 * lr).any():
                        per[name] = (int((err > 0.05 * lr).sum()), float(err.max()))
                    worst = max(worst, float(err.max()))
                # The clipped value loss max((R - v)^2, (R - v_clip)^2) has a discontinuous gradient where the two squares meet
                # (|R - v| = |R - v_clip| outside the clip range) and where v leaves the range (|v - v_old| = eps_clip): a sample
                # within float32 rounding of either contributes -2 (R - v) / mb or nothing to the critic's gradient, in any two
                # implementations.  Its distance from the discontinuity is computed here from the oracle's own values; a step
                # with such a sample may differ on the critic tensors by that one sample's share (seen: 171 weights of
                # critic.fc.0.weight at 0.06 - 0.26 lr, ragged case, step 1); every other step holds 99.99 %.
                with torch.no_grad():
                    full = {key: sn['w'][key.replace('critic.feature_net.', 'actor.feature_net.')] for key in sd
                            if not key.startswith('_actor_critic.') and not key.startswith('identifier.')}
                    ii = torch.from_numpy(sn['idx']).long()
                    v = po.critic_value(full, torch.from_numpy(obs.reshape(n, 780))[ii]).flatten().double()
                v_old = torch.from_numpy(sn['inter']['v_s'])[ii].double()
                R = torch.from_numpy(sn['inter']['returns'])[ii].double()
                v_clip = v_old + (v - v_old).clamp(-0.2, 0.2)
                outside = (v - v_old).abs() > 0.2
                margin = ((v - v_old).abs() - 0.2).abs()
                margin = torch.minimum(margin, torch.where(outside, ((R - v).abs() - (R - v_clip).abs()).abs(), torch.full_like(v, 1e9)))
                on_edge = bool((margin < 2e-6).any())
                critic_bad = sum(c for nm, (c, _) in per.items() if nm.startswith('critic.') and '.feature_net.' not in nm)
                if on_edge:
                    edge_steps.append((T, N, it, k, float(margin.min())))
                    assert n_bad - critic_bad <= 1e-4 * n_el and critic_bad <= 2e-3 * n_el, (T, N, it, k, n_bad, critic_bad, n_el, per)
                else:
                    if n_bad > 1e-4 * n_el:
                        o = f.offsets[[t[0] for t in f.table].index('critic.fc.0.weight')]
                        got = f.flat_p[o:o + 128 * 1280].cpu().numpy().reshape(128, 1280)
                        e2 = np.abs(got - post['critic.fc.0.weight'].numpy())
                        print('DIAG margin', float(margin.min()), 'sorted margins', np.sort(margin.numpy())[:5], 'rows', np.unique(np.where(e2 > 0.05 * lr)[0]),
                              'cols', np.unique(np.where(e2 > 0.05 * lr)[1])[:20], 'stats', stats.cpu().numpy(), rows[k])
                    assert n_bad <= 1e-4 * n_el, (T, N, it, k, n_bad, n_el)
            assert worst <= 2.0 * lr * 1.001
            assert len(edge_steps) <= 2, edge_steps            # the exception must stay an exception


def test_collect_train_update_cycle(M):
    """End to end on synthetic tables: collect 16 steps x 64 envs, train identifier, relabel, PPO update (2 x 2 minibatches);
    buffer invariants + finite, changing parameters; identifier loss decreases over cycles."""
    torch.manual_seed(0)
    np.random.seed(0)
    sd = po.make_policy_state_dict(5)
    pol = build_policy(M, sd)
    T = M.env.EnvTables.synthetic('cuda', n_video=4, n_user=3, n_trace=5, seed=1, n_sample=64)
    venv = M.env.MANSYVecEnv(T, 64, seed=5)
    col = M.ppo.VecCollector(pol, venv, seed=5)
    buf = M.ppo.RolloutBuffer(16, 64, 'cuda')
    p0 = pol.engine.ac.flat_p.clone()
    id_losses = []
    for cycle in range(3):
        info = col.collect(16 * 64, buf)
        assert info['n/st'] == 1024 and len(buf) == 1024
        # transition chaining: where not done, next step's obs is this step's obs_next
        nd = buf.done[:-1] == 0
        assert torch.equal(buf.obs[1:][nd], buf.obs_next[:-1][nd])
        a, b = 748, 763
        onehot = buf.obs_next[..., a:b]
        assert torch.equal(onehot.argmax(-1).int(), buf.act) and (onehot.sum(-1) == 1).all()
        losses, vloss = pol.train_identifier(buf, 2, verbose=False)
        id_losses.append(losses[0].item())
        res = pol.update(0, buf, is_train=True, batch_size=256, repeat=2)
        assert len(res['loss']) == 8 and np.isfinite(res['loss']).all(), res
        assert 0 < np.mean(res['loss/ent']) <= np.log(15) + 1e-4
    assert torch.isfinite(pol.engine.ac.flat_p).all() and not torch.equal(p0, pol.engine.ac.flat_p)
    assert id_losses[-1] < id_losses[0]


def test_behaviour_cloning_steps_then_ppo_with_per_parameter_adam_steps(M):
    """behavior_cloning_pretraining's step (CE - 0.1 * entropy, Adam(L2) on the parameters that have gradients) followed by
    PPO minibatch steps: torch.optim.Adam keeps one step counter per parameter, so the critic head (no gradient during
    cloning) starts at step 1 when PPO begins.  Oracle = torch autograd + torch.optim.Adam on oracle/ppo_oracle.py."""
    from mansy_immersivevideostreaming_amd._lib import check, lib, ptr, stream_ptr
    sd = po.make_policy_state_dict(int(Z['wseed']))
    pol = build_policy(M, sd)
    uniq, params = {}, {}
    for k, v in sd.items():
        if k.startswith('_actor_critic.') or k.startswith('identifier.'):
            continue
        key = k.replace('critic.feature_net.', 'actor.feature_net.')
        if key not in uniq:
            uniq[key] = v.clone().requires_grad_(True)
        params[k] = uniq[key]
    opt = torch.optim.Adam(list(uniq.values()), lr=5e-4, weight_decay=1e-2)
    g = torch.Generator().manual_seed(21)
    eng, f = pol.engine, pol.engine.ac
    names = [n for n, _ in f.table]

    def compare(tag, atol):
        # Adam divides by sqrt(v): elements whose gradient is at rounding-noise level move by up to lr per step in either
        # implementation, so a handful of outliers (< 0.01 %) are allowed up to a fraction of lr
        for n_, o, p in zip(names, f.offsets, f.params):
            got = f.flat_p[o:o + p.numel()].view(p.shape).cpu().numpy()
            want = uniq[n_].detach().numpy()
            err = np.abs(got - want)
            assert (err > atol).mean() <= 1e-4 and err.max() <= 2.5e-4, (tag, n_, (err > atol).sum(), err.max())

    n_bc = 4
    for k in range(n_bc):
        n = [51, 33, 1, 64][k]                       # demonstrations have different lengths; a single transition is legal
        obs = torch.from_numpy(Z['obs'][50 * k:50 * k + n])
        act = torch.randint(0, 15, (n,), generator=g)
        opt.zero_grad(set_to_none=True)
        loss, ce, ent = po.bc_loss(po.actor_logits(params, obs), act)
        loss.backward()
        assert uniq['critic.fc.0.weight'].grad is None
        opt.step()
        stats = pol.bc_step(obs.cuda(), act.int().cuda(), ent_coef=0.1, train=True).cpu().numpy()
        np.testing.assert_allclose(stats, [loss.item(), ce.item(), ent.item()], rtol=3e-5, atol=3e-6)
    assert f.step == n_bc and f.tail() == (f.offsets[names.index('critic.fc.0.weight')], 0)
    compare('after cloning', 2e-6)
    np.testing.assert_array_equal(f.params[names.index('critic.fc.0.weight')].detach().cpu().numpy(), sd['critic.fc.0.weight'].numpy())
    # validation pass: plain cross entropy, nothing moves
    before = f.flat_p.clone()
    obs = torch.from_numpy(Z['obs'][205:245])
    act = torch.randint(0, 15, (40,), generator=g)
    with torch.no_grad():
        _, ce, _ = po.bc_loss(po.actor_logits(params, obs), act)
    st = pol.bc_step(obs.cuda(), act.int().cuda(), train=False).cpu().numpy()
    np.testing.assert_allclose(st[1], ce.item(), rtol=3e-5)
    assert torch.equal(before, f.flat_p) and f.step == n_bc
    # PPO minibatch steps on top: clip_grad_norm_ + Adam with the critic head lagging by n_bc steps
    obs, act, adv, v_old, ret, g2 = _minibatch_data()
    with torch.no_grad():
        logp_old = torch.log_softmax(po.actor_logits(params, obs), -1).gather(1, act[:, None])[:, 0] + 0.2 * torch.randn(len(obs), generator=g2)
    d = dict(obs=obs.cuda(), act=act.int().cuda(), adv=adv.cuda(), logp=logp_old.cuda(), v=v_old.cuda(), ret=ret.cuda())
    stats = torch.zeros(4, device='cuda')
    for k in range(3):
        opt.zero_grad(set_to_none=True)
        loss, *_ = po.ppo_loss(po.actor_logits(params, obs), po.critic_value(params, obs), act, adv, logp_old, v_old, ret)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(list(uniq.values()), 1.0)
        opt.step()
        f.step += 1
        arr, garr = f.pointers(grads=True)
        assert f.tail()[1] == k + 1
        check(lib().mansy_ppo_minibatch_step(arr, garr, ptr(f.flat_p), ptr(f.flat_g), ptr(f.m), ptr(f.v), f.flat_p.numel(), ptr(d['obs']), None,
                                             ptr(d['act']), ptr(d['adv']), ptr(d['logp']), ptr(d['v']), ptr(d['ret']), len(obs), 0.2, 0.5, 0.02, 1, 1, 0.0,
                                             1.0, 5e-4, 1e-2, f.step, *f.tail(), ptr(stats), ptr(eng.workspace()), eng.max_batch, 0, None, 0, None, None, eng.prec, stream_ptr()),
              'ppo_mb')
        np.testing.assert_allclose(stats[0].item(), loss.item(), rtol=5e-5, atol=5e-6)
    compare('after PPO steps', 6e-6)
    # the same three steps WITHOUT the lag would have moved the critic head differently (the test has teeth)
    k = names.index('critic.out.weight')
    moved = (f.params[k].detach().cpu() - sd['critic.out.weight']).abs().max().item()
    assert moved > 1e-3            # first Adam steps of a fresh parameter are ~lr each


def test_fused_rollout_step_equals_policy_forward_plus_env_step(M):
    """mansy_policy_env_step (sampling + environment step in the output-layer launch) against the two separate calls on the
    same observations and uniforms, through episode ends: actions, log-probs, observations, rewards, done flags bit-identical."""
    sd = po.make_policy_state_dict(int(Z['wseed']))
    pol = build_policy(M, sd)
    eng = pol.engine
    T = M.env.EnvTables.synthetic('cuda', n_video=5, n_user=4, n_trace=6, n_chunk=60, seed=3, n_sample=37, train_identifier_reward=True)
    N = 192
    va, vb = M.env.MANSYVecEnv(T, N, seed=4), M.env.MANSYVecEnv(T, N, seed=4)
    oa, ob = va.reset().clone(), vb.reset().clone()
    assert torch.equal(oa, ob)
    g = torch.Generator(device='cuda').manual_seed(1)
    f32 = dict(dtype=torch.float32, device='cuda')
    act_b, logp_b = torch.empty(N, dtype=torch.int32, device='cuda'), torch.empty(N, **f32)
    nxt_b, on_b, rew_b = torch.empty(N, 780, **f32), torch.empty(N, 780, **f32), torch.empty(N, **f32)
    done_b = torch.empty(N, dtype=torch.uint8, device='cuda')
    n_done = 0
    for t in range(70):
        u = torch.rand(N, generator=g, **f32)
        _, _, act_a, logp_a = eng.policy_forward(oa, want_value=False, sample=True, u=u)
        cur_a, rew_a, done_a, _ = va.step(act_a)
        eng.policy_env_step(vb, ob, u, act_b, logp_b, nxt_b, on_b, rew_b, done_b, reuse_packed=t > 0)
        assert torch.equal(act_a, act_b) and torch.equal(logp_a, logp_b), t
        assert torch.equal(rew_a, rew_b) and torch.equal(done_a, done_b), t
        assert torch.equal(va.obs_next, on_b) and torch.equal(cur_a, nxt_b), t
        assert torch.equal(va.state, vb.state), t
        n_done += int(done_a.sum())
        oa, ob = cur_a.clone(), nxt_b.clone()
    assert n_done >= N
    np.testing.assert_array_equal(va.pop_episode_log()[:, [0, 2, 7]].sum(0), vb.pop_episode_log()[:, [0, 2, 7]].sum(0))


@pytest.mark.parametrize('N,Tsteps', [(256, 16), (100, 7), (32, 3)])
def test_persistent_rollout_on_xcd_teams_equals_the_per_step_launches(M, N, Tsteps):
    """Round 5: a whole collect as ONE persistent launch (mansy_policy_rollout: one workgroup per CU, a team per XCD read from HW_REG_XCC_ID, the three
    launches of a step as three phases separated by barriers through the XCD's L2; the chunks of 32 environments never leave their team) against the
    per-step launches on the same uniforms, through episode ends and auto-resets, several collects in a row (the control block is re-zeroed, the packed
    weights re-built, the carry handed over): every slab of the rollout buffer, the carry, the environment records and the episode log bit-identical.
    Ragged sizes: a last chunk of 4 rows, fewer chunks than teams."""
    sd = po.make_policy_state_dict(int(Z['wseed']))
    tables = M.env.EnvTables.synthetic('cuda', n_video=5, n_user=4, n_trace=6, n_chunk=30, seed=3, n_sample=max(37, N), train_identifier_reward=True)
    out = {}
    for form in ('team', 'steps'):
        pol = build_policy(M, sd)
        venv = M.env.MANSYVecEnv(tables, N, seed=4)
        col = M.ppo.VecCollector(pol, venv, seed=5, use_graph=False)
        col.use_team = form == 'team'
        buf = M.ppo.RolloutBuffer(Tsteps, N, 'cuda')
        torch.manual_seed(11)
        snaps = []
        for it in range(4):
            col.collect(Tsteps * N, buf)
            torch.cuda.synchronize()
            snaps.append([t.clone() for t in (buf.obs, buf.obs_next, buf.act, buf.logp, buf.rew, buf.done, col.carry, venv.state)])
        assert col.use_team == (form == 'team')                       # the library took the persistent form (no silent per-step path)
        if form == 'team':
            assert int(pol.engine._rollout_err[0]) == 0
        out[form] = (snaps, venv.pop_episode_log())
    n_done = 0
    for a, b in zip(out['team'][0], out['steps'][0]):
        for x, y in zip(a, b):
            assert torch.equal(x, y)
        n_done += int(a[5].sum())
    if 4 * Tsteps >= 28:
        assert n_done >= N // 2                                       # episodes did end (30-chunk videos): auto-resets were exercised
    la, lb = out['team'][1], out['steps'][1]
    assert la.shape == lb.shape and len(la) == n_done
    np.testing.assert_array_equal(la[np.lexsort(la.T[::-1])], lb[np.lexsort(lb.T[::-1])])      # (records are appended in completion order: compare as sets)


def test_behavior_cloning_pretraining_vs_reference(M, tmp_path):
    """The whole behavior_cloning_pretraining() loop (utils/mansy_utils.py:52-93) against the capture of the IMPORTED reference
    function (tools/gen_golden_bc.py: duck-typed policy around the reference Actor, duck-typed demonstrations): same host RNG
    stream (random.choice picks the demonstration, np.random.shuffle inside train_identifier), per-step losses, validation
    losses, best-step choice and the saved best checkpoint, interleaved identifier training, resulting weights."""
    import contextlib
    import io
    import random
    from mansy_immersivevideostreaming_amd.bitrate_selection.utils.mansy_utils import behavior_cloning_pretraining
    G = _golden.load(os.path.join(os.path.dirname(__file__), 'golden', 'bc_reference.npz'))
    sd = po.make_policy_state_dict(int(G['wseed']))
    pol = build_policy(M, sd, lr=float(G['lr']), ilr=float(G['ilr']), wd=float(G['wd']))
    nt, nv = int(G['n_train']), int(G['n_valid'])
    demos = [{'obs': G[f'demo{i}/obs'], 'act': G[f'demo{i}/act']} for i in range(nt + nv)]
    seed = int(G['seed'])
    random.seed(seed); np.random.seed(seed); torch.manual_seed(seed)
    ppath, ipath = str(tmp_path / 'p.pth'), str(tmp_path / 'i.pth')

    class A:
        device = 'cuda'
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        best_loss, best_step = behavior_cloning_pretraining(A(), pol, pol.identifier, pol.optim, pol.identifier_optim, demos[:nt], demos[nt:],
                                                            int(G['max_steps']), int(G['valid_per_step']), int(G['id_max_steps']),
                                                            int(G['id_rounds']), ppath, ipath)
    lines = out.getvalue().splitlines()
    tr = [float(l.split('loss=')[1].split(' ')[0]) for l in lines if l.startswith('BC (Training)')]
    va = [(float(l.split('valid loss=')[1].split(' ')[0]), float(l.split('best loss=')[1].split(' ')[0]), int(l.rsplit(' ', 1)[1]))
          for l in lines if l.startswith('BC (Validation)')]
    np.testing.assert_allclose(tr, G['train_losses'], rtol=1e-4)
    np.testing.assert_allclose([v[0] for v in va], G['valid_losses'], rtol=1e-4)
    np.testing.assert_allclose([v[1] for v in va], G['best_losses'], rtol=1e-4)
    assert [v[2] for v in va] == G['best_steps'].tolist() and best_step == int(G['best_steps'][-1])
    np.testing.assert_allclose(best_loss, G['best_losses'][-1], rtol=1e-4)
    idl = [float(l.split(':')[-1]) for l in lines if 'identifier loss is' in l]
    idv = [float(l.split(':')[-1]) for l in lines if 'identifier validation loss is' in l]
    np.testing.assert_allclose(idl, G['ident_train_losses'], rtol=2e-4)
    np.testing.assert_allclose(idv, G['ident_valid_losses'], rtol=2e-4)

    def cut(t):
        v2 = t.detach().cpu().numpy().reshape(t.shape[0], -1)
        return v2[::5, ::7] if v2.size > 20000 else v2

    def close(got, want, key, lr, steps):
        # Adam moves every weight by up to lr per step in the direction of sign(g): elements whose gradient is at rounding-noise
        # level may differ by a few lr between two implementations; everything else agrees to a fraction of lr
        err = np.abs(got - want)
        assert (err > 0.05 * lr).mean() <= 0.02 and err.max() <= 2.2 * lr * steps, (key, float((err > 0.05 * lr).mean()), float(err.max()))
    after, best = pol.state_dict(), torch.load(ppath)
    n_steps = int(G['max_steps'])
    for key in G.files:
        if key.startswith('after::actor.') or key.startswith('after::critic.'):
            close(cut(after[key[7:]]), G[key], key, float(G['lr']), n_steps)
        if key.startswith('after::critic.'):                     # no gradient during cloning: untouched, bit for bit
            assert torch.equal(after[key[7:]].cpu(), sd[key[7:]]), key
        if key.startswith('best::actor.'):
            close(cut(best[key[6:]]), G[key], key, float(G['lr']), int(G['best_steps'][-1]) + 1)
        if key.startswith('after::identifier.'):
            close(cut(after[key[7:]]), G[key], key, float(G['ilr']), int(G['id_max_steps']) * int(G['id_rounds']))
        if key.startswith('norm::actor.'):
            np.testing.assert_allclose(after[key[6:]].double().norm().item(), float(G[key]), rtol=2e-4, err_msg=key)
    assert os.path.exists(ipath)


def test_whole_update_vs_oracle_update(M):
    """PPOPolicy.update(0, buffer, is_train=True, batch_size=512, repeat=2) end to end against oracle.ppo_oracle.update -- the
    reference's order of operations (mansy_ppo.py:36-59: relabel -> process_fn -> learn) on a fixed buffer and a fixed np.random
    seed, TWO consecutive updates (so the return normaliser and the Adam moments carry over): the relabelled rewards, the
    minibatch split order (np.random.permutation, merge_last: 4096 = 8 x 512 per pass, and a ragged 1100 = 512 + 588 case), the
    loss rows, every weight after the update and the ret_rms state.

    The first pass of the first update agrees to rounding, and so does everything each update starts from (relabelled rewards,
    return normaliser, first row); later rows and the final weights are compared loosely.  The clipped value loss max((R - v)^2, (R - v_clip)^2) has a DISCONTINUOUS gradient: once the
    values have moved more than eps_clip from v_old (all 512 samples of most minibatches here), a sample contributes -2 (R - v)
    or nothing depending on which square is larger, so a 1e-6 difference in v flips a sample at the boundary and moves the
    gradient of a minibatch in which only ~35 samples contribute by several per cent -- in any two fp32 implementations
    (tools/ppo_update_probe.py: the engine's per-sample rule equals autograd's on every sample; the first flip appears at step 26)."""
    sd = po.make_policy_state_dict(int(Z['wseed']))
    for (T, N, bs) in ((16, 256, 512), (11, 100, 512)):
        pol = build_policy(M, sd)
        rs = np.random.RandomState(3)
        n = T * N
        src = Z['obs']
        obs = src[rs.randint(0, len(src), size=n)].reshape(T, N, 780).copy()
        obs_next = src[rs.randint(0, len(src), size=n)].reshape(T, N, 780).copy()
        act = rs.randint(0, 15, size=(T, N)).astype(np.int32)
        rew = rs.randn(T, N).astype(np.float32)
        done = rs.rand(T, N) < 0.05
        buf = M.ppo.RolloutBuffer(T, N, 'cuda')
        rms_o, ost = po.RunningMeanStd(), {}
        for it in range(2):
            r_it = rew + 0.1 * it
            buf.obs.copy_(torch.from_numpy(obs)); buf.obs_next.copy_(torch.from_numpy(obs_next)); buf.act.copy_(torch.from_numpy(act))
            buf.rew.copy_(torch.from_numpy(r_it)); buf.done.copy_(torch.from_numpy(done.astype(np.uint8)))
            buf.filled = T
            np.random.seed(100 + it)
            res = pol.update(0, buf, is_train=True, batch_size=bs, repeat=2)
            got_rows = np.stack([res['loss'], res['loss/clip'], res['loss/vf'], res['loss/ent']], 1)
            np.random.seed(100 + it)
            sd_now = {k: v.clone() for k, v in sd.items()}                   # identifier weights are not touched by update()
            want_rows, inter = po.update(sd_now, obs, obs_next, act, r_it, done, rms_o, ost, lamb=0.5, batch_size=bs, repeat=2)
            assert got_rows.shape == want_rows.shape == ((16, 4) if n == 4096 else (4, 4))
            np.testing.assert_allclose(buf.rew.cpu().numpy().reshape(-1), inter['rew'], atol=2e-6, rtol=0)          # relabel, in place
            # ret_rms absorbs the un-normalised returns of the whole buffer: pins process_fn (values, GAE, normalisation order)
            # (the second update starts from weights that may already differ by a flipped sample: 1e-2)
            np.testing.assert_allclose(pol.ret_rms().cpu().numpy(), [rms_o.mean, rms_o.var, rms_o.count], rtol=2e-6 if it == 0 else 1e-2)
            tight = dict(rtol=1e-5, atol=3e-6)
            first_pass = len(got_rows) // 2
            if it == 0:          # first pass of the first update: ratio == 1 and |v - v_old| small at its start -> no flips yet
                np.testing.assert_allclose(got_rows[:2], want_rows[:2], **tight)
                np.testing.assert_allclose(got_rows[:first_pass], want_rows[:first_pass], rtol=2e-4, atol=2e-5)
            np.testing.assert_allclose(got_rows, want_rows, rtol=3e-2, atol=2e-3)
            f = pol.engine.ac
            for name, o, p in zip([t[0] for t in f.table], f.offsets, f.params):
                got = f.flat_p[o:o + p.numel()].view(p.shape).cpu().numpy()
                want = ost['uniq'][name].detach().numpy()
                err = np.abs(got - want)
                # Adam moves a weight by up to lr per step whatever the gradient's size: after a flipped sample the two trajectories
                # differ by a fraction of lr per step on most weights and by up to 2 lr per step on a few
                steps = len(got_rows) * (it + 1)
                assert err.max() <= steps * 2 * 5e-4 and np.median(err) <= 1e-4, (T, N, it, name, float(np.median(err)), float(err.max()))


def test_chained_update_equals_self_contained_steps(M):
    """learn() chains the minibatch steps: a step's last launch (clip + Adam) also zeroes the gradients, scatters the updated
    parameters into the packed block-diagonal / stacked images and gathers the next minibatch; the next step skips its prologue
    launch.  Same values in the same places: two updates (4096 transitions, and a ragged 1100 with merge_last) must leave every
    weight, Adam moment and loss row where the self-contained steps leave them -- to float32 rounding, not bit for bit: the
    output-layer backward adds its per-workgroup partial sums with float atomics, whose order varies from launch to launch
    (measured: loss rows of two chained-vs-unchained runs differ by <= 2.4e-7, the first step is identical)."""
    sd = po.make_policy_state_dict(int(Z['wseed']))
    for (T, N, bs) in ((16, 256, 512), (11, 100, 512)):
        rs = np.random.RandomState(7)
        n = T * N
        src = Z['obs']
        obs = torch.from_numpy(src[rs.randint(0, len(src), size=n)].reshape(T, N, 780).copy())
        obs_next = torch.from_numpy(src[rs.randint(0, len(src), size=n)].reshape(T, N, 780).copy())
        act = torch.from_numpy(rs.randint(0, 15, size=(T, N)).astype(np.int32))
        rew = torch.from_numpy(rs.randn(T, N).astype(np.float32))
        done = torch.from_numpy((rs.rand(T, N) < 0.05).astype(np.uint8))
        outs = []
        for chained in (True, False):
            pol = build_policy(M, sd)
            pol.chain_steps = chained
            buf = M.ppo.RolloutBuffer(T, N, 'cuda')
            rows = []
            for it in range(2):
                buf.obs.copy_(obs); buf.obs_next.copy_(obs_next); buf.act.copy_(act); buf.rew.copy_(rew + 0.1 * it); buf.done.copy_(done)
                buf.filled = T
                np.random.seed(50 + it)
                res = pol.update(0, buf, is_train=True, batch_size=bs, repeat=2)
                rows.append(np.stack([res['loss'], res['loss/clip'], res['loss/vf'], res['loss/ent']], 1))
            f = pol.engine.ac
            outs.append((np.concatenate(rows), f.flat_p.clone(), f.m.clone(), f.v.clone()))
        np.testing.assert_array_equal(outs[0][0][0], outs[1][0][0])              # first step: the same prologue launch either way
        np.testing.assert_allclose(outs[0][0], outs[1][0], rtol=2e-5, atol=2e-6)
        for a, b in zip(outs[0][1:], outs[1][1:]):
            err = (a - b).abs()
            assert float((err > 0.02 * 5e-4).float().mean()) <= 1e-4 and err.max().item() <= 2 * 5e-4, (err.max().item(),)
        assert np.isfinite(outs[0][0]).all() and len(outs[0][0]) == (32 if n == 4096 else 8)


def test_data_parallel_step_form_equals_the_single_process_step(M):
    """The data-parallel form of an update -- raw gradients (step = 0), average over the ranks, then mansy_ppo_dp_tail (clip + Adam +
    gradient zero-fill + re-pack + next minibatch's gather) or, unchained, mansy_clip_grad_adam -- with an identity `grad_sync`
    (one rank) must land where the single-process chained step lands: same gradients, same clip, same Adam, to float32 rounding.
    Round 5: also the peer-memory forms on a one-rank context with the average REALLY issued -- 'peer-slot' (the default: the whole
    data-parallel step is one mansy_ppo_minibatch_step(..., xg_ctx) call, gradients produced in the exchange slot, one launch publishes /
    waits / sums) and 'peer-copy' (the round-4 three-call form) -- and the identifier's training rounds in the same two forms."""
    sd = po.make_policy_state_dict(int(Z['wseed']))
    T, N, bs = 11, 100, 512                                         # ragged: 512 + 588 per pass
    rs = np.random.RandomState(11)
    n = T * N
    src = Z['obs']
    obs = torch.from_numpy(src[rs.randint(0, len(src), size=n)].reshape(T, N, 780).copy())
    obs_next = torch.from_numpy(src[rs.randint(0, len(src), size=n)].reshape(T, N, 780).copy())
    act = torch.from_numpy(rs.randint(0, 15, size=(T, N)).astype(np.int32))
    rew = torch.from_numpy(rs.randn(T, N).astype(np.float32))
    done = torch.from_numpy((rs.rand(T, N) < 0.05).astype(np.uint8))
    outs = []
    ident = []
    from mansy_immersivevideostreaming_amd import dist as mdist
    comms = []
    for form in ('single', 'dp-chained', 'dp-unchained', 'peer-slot', 'peer-copy', 'peer-slot-unchained', 'rccl-comm'):
        pol = build_policy(M, sd)
        if form == 'rccl-comm':      # the library's own RCCL communicator (mansy_comm_* / mansy_allreduce_avg_f32) as the step's sync context: one call per step
            comms.append(mdist.RcclComm(1, 0, torch.device('cuda', torch.cuda.current_device())))
            pol.set_data_parallel(1, None, force=True, comm=comms[-1])
            assert pol._xg_ctx(pol.engine.ac) is not None
        elif form.startswith('peer'):
            pol.peer_in_slot = form != 'peer-copy'
            pol.set_data_parallel(1, None, peer=True, force=True)
            pol.chain_steps = form != 'peer-slot-unchained'            # unchained: the slot form is not available, the copy form takes over on the same context
            assert (pol._xg_ctx(pol.engine.ac) is not None) == (form != 'peer-copy')
        elif form != 'single':
            pol.set_data_parallel(1, lambda g: None)
            pol.chain_steps = form == 'dp-chained'
        buf = M.ppo.RolloutBuffer(T, N, 'cuda')
        rows = []
        for it in range(2):
            buf.obs.copy_(obs); buf.obs_next.copy_(obs_next); buf.act.copy_(act); buf.rew.copy_(rew + 0.1 * it); buf.done.copy_(done)
            buf.filled = T
            np.random.seed(70 + it)
            res = pol.update(0, buf, is_train=True, batch_size=bs, repeat=2)
            rows.append(np.stack([res['loss'], res['loss/clip'], res['loss/vf'], res['loss/ent']], 1))
        f = pol.engine.ac
        outs.append((np.concatenate(rows), f.flat_p.clone(), f.m.clone(), f.v.clone()))
        if form in ('single', 'peer-slot', 'peer-copy', 'rccl-comm'):            # train_identifier: two full-batch rounds + validation, same shuffle
            np.random.seed(5)
            losses, vloss = pol.train_identifier(buf, 2, verbose=False)
            torch.cuda.synchronize()
            pol._check_peers()
            ident.append((np.array([l.item() for l in losses] + [vloss.item()]), pol.engine.idn.flat_p.clone()))
    for cm in comms:
        cm.close()
    for losses, flat in ident[1:]:
        np.testing.assert_allclose(losses, ident[0][0], rtol=1e-6, atol=1e-7)
        assert (flat - ident[0][1]).abs().max().item() <= 2.1 * 1e-4          # Adam(lr 1e-4): +-lr steps of zero-gradient parameters at most
        assert float(((flat - ident[0][1]).abs() > 1e-6).float().mean()) <= 2e-3
    for o in outs[1:]:
        np.testing.assert_allclose(o[0], outs[0][0], rtol=2e-5, atol=2e-6)
        for a, b in zip(o[1:], outs[0][1:]):
            err = (a - b).abs()
            assert float((err > 0.02 * 5e-4).float().mean()) <= 1e-4 and err.max().item() <= 2 * 5e-4, (err.max().item(),)


def test_identifier_gradient_averages_hidden_under_process_fn_passes(M):
    """Data parallel: the two gradient averages of train_identifier run on a side stream while the two
    evaluation passes of the following process_fn (v_s + logp_old on obs; v_s_ on obs_next -- they depend on the actor-critic only)
    run on the caller's stream; process_fn then takes those values instead of recomputing them.  With an identity `grad_sync` (one
    rank) the whole collect-less cycle train_identifier -> update must land where the un-overlapped order lands: same identifier
    losses and parameters, same PPO losses and parameters, to float32 rounding (the two halves are evaluated as two passes instead
    of one joint pass: a different split of the fc product's batch, nothing else); a stale cache (other buffer, changed policy) is
    never used."""
    sd = po.make_policy_state_dict(int(Z['wseed']))
    T, N, bs = 16, 64, 256
    rs = np.random.RandomState(5)
    n = T * N
    src = Z['obs']
    obs2 = torch.from_numpy(src[rs.randint(0, len(src), size=2 * n)].reshape(2, T, N, 780).copy())
    act = torch.from_numpy(rs.randint(0, 15, size=(T, N)).astype(np.int32))
    rew = torch.from_numpy(rs.randn(T, N).astype(np.float32))
    done = torch.from_numpy((rs.rand(T, N) < 0.05).astype(np.uint8))
    outs = []
    for hide in (False, True):
        pol = build_policy(M, sd)
        calls = []
        pol.set_data_parallel(1, lambda g: calls.append(g.numel()))
        pol.overlap_identifier_sync = hide
        buf = M.ppo.RolloutBuffer(T, N, 'cuda')
        rows, ilosses = [], []
        for it in range(2):
            buf.obs.copy_(obs2[0]); buf.obs_next.copy_(obs2[1]); buf.act.copy_(act); buf.rew.copy_(rew + 0.1 * it); buf.done.copy_(done)
            buf.filled = T
            np.random.seed(90 + it)
            il, vl = pol.train_identifier(buf, 2, verbose=False)
            assert (pol._pre_eval is not None and pol._pre_eval['done'] == {0, 1}) == hide
            ilosses += [x.item() for x in il] + [vl.item()]
            res = pol.update(0, buf, is_train=True, batch_size=bs, repeat=2)
            assert pol._pre_eval is None                                  # consumed (or never there)
            rows.append(np.stack([res['loss'], res['loss/clip'], res['loss/vf'], res['loss/ent']], 1))
        assert calls.count(pol.engine.idn.flat_p.numel()) == 4          # the identifier's 2 x 2 averages went through grad_sync either way
        outs.append((np.array(ilosses), np.concatenate(rows), pol.engine.idn.flat_p.clone(), pol.engine.ac.flat_p.clone()))
        if hide:      # a cache taken for another buffer state must not be used: process_fn recomputes
            pol._pre_evaluate(buf, 0)
            buf.filled = T - 1
            data = pol.process_fn(buf)
            assert data['n'] == (T - 1) * N and pol._pre_eval is None
    np.testing.assert_allclose(outs[1][0], outs[0][0], rtol=1e-6)
    np.testing.assert_allclose(outs[1][1], outs[0][1], rtol=2e-5, atol=2e-6)
    ierr = (outs[1][2] - outs[0][2]).abs()                               # identifier: the same launches (bias-gradient row sums are float atomics: rounding noise, which Adam turns into +-lr on zero-gradient elements)
    assert float((ierr > 0.02 * 1e-4).float().mean()) <= 1e-3 and ierr.max().item() <= 4 * 1e-4, ierr.max().item()
    err = (outs[1][3] - outs[0][3]).abs()
    assert float((err > 0.02 * 5e-4).float().mean()) <= 1e-4 and err.max().item() <= 2 * 5e-4, err.max().item()


@pytest.mark.parametrize('mode', ['f32', 'bf16x6', 'bf16x3'])
def test_shipped_trained_checkpoint_vs_reference(M, mode):
    """The TRAINED weights the reference ships (best_policy.pth / best_identifier.pth; their arrays travel in
    tests/golden/shipped_checkpoint_reference.npz, tools/gen_golden_shipped.py) through the HIP nets on real observations against
    the imported reference: logits / values / identifier outputs within 1e-4, every argmax (bitrate) decision identical, the
    un-batched identifier reward -- in the exact-fp32 mode and in both split-bf16 modes."""
    from mansy_immersivevideostreaming_amd import kernels
    G = _golden.load(os.path.join(os.path.dirname(__file__), 'golden', 'shipped_checkpoint_reference.npz'))
    assert int(G['shared_feature_net_identical']) == 1
    uniq = {k[3:]: torch.from_numpy(G[k]) for k in G.files if k.startswith('w::')}
    sd = {}
    for k in po.make_policy_state_dict(0):                      # the 120-key layout of the shipped checkpoint
        src = k.replace('_actor_critic.', '')
        src = src.replace('critic.feature_net.', 'actor.feature_net.')
        sd[k] = uniq[src]
    pol = build_policy(M, sd)
    obs = torch.from_numpy(G['obs']).cuda()
    with kernels.precision(mode):
        logits, _ = pol.actor(obs)
        value = pol.critic(obs)
        pred = pol.identifier(obs)
        buf = M.ppo.RolloutBuffer(8, 1, 'cuda')
        buf.obs[:, 0] = obs[:8]
        buf.rew[:, 0] = 0.0
        buf.filled = 8
        pol.relabel(buf, lamb=1.0)                               # rew <- identifier reward
    tol = 2e-5 if mode != 'bf16x3' else 1e-4
    np.testing.assert_allclose(logits.cpu().numpy(), G['logits'], atol=tol, rtol=0)
    np.testing.assert_allclose(value.cpu().numpy(), G['value'], atol=tol, rtol=0)
    np.testing.assert_allclose(pred.cpu().numpy(), G['ident'], atol=tol, rtol=0)
    assert (logits.argmax(-1).cpu().numpy() == G['logits'].argmax(-1)).all()
    np.testing.assert_allclose(buf.rew[:, 0].cpu().numpy(), G['ident_reward'], atol=tol, rtol=0)


@pytest.mark.parametrize('form', ['single', 'peer-slot', 'rccl-comm-forced'])
def test_graph_replayed_update_half_equals_direct_launches(M, form):
    """Round 6: train_identifier() and update() replayed from captured hipGraphs (PPOPolicy.graph_update: first call direct, second call capture +
    replay, then replays) against the same calls as direct launches, four cycles each on the same buffer contents and the same numpy seeds.
    What a replay cannot take from its frozen kernel arguments comes from device memory: the permutations / the identifier's shuffle (staged
    upload), the Adam bias corrections of the replay's step counts (`adam_bias`), the peer-memory epoch (derived from the rank's own flag word).
    Same launches on the same data: loss rows, weights, Adam moments, return normaliser and identifier agree to float32 rounding (float atomics
    in the bias-gradient sums order differently from run to run) -- and the step counters, which are host state, agree exactly."""
    from mansy_immersivevideostreaming_amd import dist as mdist
    sd = po.make_policy_state_dict(int(Z['wseed']))
    T, N, bs = 16, 256, 512
    rs = np.random.RandomState(21)
    n = T * N
    src = Z['obs']
    obs = torch.from_numpy(src[rs.randint(0, len(src), size=n)].reshape(T, N, 780).copy())
    obs_next = torch.from_numpy(src[rs.randint(0, len(src), size=n)].reshape(T, N, 780).copy())
    act = torch.from_numpy(rs.randint(0, 15, size=(T, N)).astype(np.int32))
    rew = torch.from_numpy(rs.randn(T, N).astype(np.float32))
    done = torch.from_numpy((rs.rand(T, N) < 0.05).astype(np.uint8))
    outs, comms = [], []
    for graph in (False, 'auto'):
        pol = build_policy(M, sd)
        if form == 'peer-slot':
            pol.set_data_parallel(1, None, peer=True, force=True, in_slot=True)
        elif form == 'rccl-comm-forced':
            comms.append(mdist.RcclComm(1, 0, torch.device('cuda', torch.cuda.current_device())))
            pol.set_data_parallel(1, None, force=True, comm=comms[-1])
        pol.graph_update = graph if not (graph and form == 'rccl-comm-forced') else True       # a library collective inside the graph: only when forced
        buf = M.ppo.RolloutBuffer(T, N, 'cuda')
        rows, ilosses = [], []
        for it in range(4):
            buf.obs.copy_(obs); buf.obs_next.copy_(obs_next); buf.act.copy_(act); buf.rew.copy_(rew + 0.1 * it); buf.done.copy_(done)
            buf.filled = T
            np.random.seed(300 + it)
            losses, vloss = pol.train_identifier(buf, 2, verbose=False)
            res = pol.update(0, buf, is_train=True, batch_size=bs, repeat=2)
            ilosses.append([l.item() for l in losses] + [vloss.item()])
            rows.append(np.stack([res['loss'], res['loss/clip'], res['loss/vf'], res['loss/ent']], 1))
        torch.cuda.synchronize()
        pol.sync_check()
        assert pol.graph_replays == (6 if graph else 0), pol.graph_replays            # cycles 2, 3, 4 x (identifier, update)
        assert pol.engine.ac.step == 64 and pol.engine.idn.step == 8
        if graph:
            assert sorted(g['launches'] for g in pol._graphs.values())[0] >= 10
        outs.append((np.concatenate(rows), np.array(ilosses), pol.engine.ac.flat_p.clone(), pol.engine.ac.m.clone(), pol.engine.ac.v.clone(),
                     pol.engine.idn.flat_p.clone(), pol.ret_rms().clone(), buf.rew.clone()))
    for cm in comms:
        cm.close()
    a, b = outs
    np.testing.assert_array_equal(a[0][0], b[0][0])                       # first step of the first (direct) cycle: identical launches
    np.testing.assert_allclose(b[0], a[0], rtol=2e-4, atol=2e-5)          # 64 loss rows
    np.testing.assert_allclose(b[1], a[1], rtol=1e-5, atol=1e-7)          # identifier losses (8 training rounds + 4 validations)
    for x, y, lr in ((a[2], b[2], 5e-4), (a[3], b[3], 5e-4), (a[4], b[4], 5e-4), (a[5], b[5], 1e-4)):
        err = (x - y).abs()
        assert float((err > 0.02 * lr).float().mean()) <= 2e-3 and err.max().item() <= 4 * lr, (err.max().item(),)
    np.testing.assert_allclose(b[6].cpu().numpy(), a[6].cpu().numpy(), rtol=1e-4)       # return normaliser after four updates
    np.testing.assert_allclose(b[7].cpu().numpy(), a[7].cpu().numpy(), atol=5e-5)       # relabelled rewards of the last cycle


def test_graph_replay_needs_an_even_step_count_and_falls_back_otherwise(M):
    """1100 transitions at batch 512 and repeat 1 = 2 steps (even: replayed); 1536 at 512 and repeat 1 = 3 steps (odd: the norm-slot sets
    would start a replay on the other parity) -> direct launches, same results as with graph_update = False."""
    sd = po.make_policy_state_dict(int(Z['wseed']))
    src = Z['obs']
    for (T, N, want_replays) in ((11, 100, 2), (12, 128, 0)):
        got = []
        for graph in (False, 'auto'):
            rs = np.random.RandomState(4)
            n = T * N
            pol = build_policy(M, sd)
            pol.graph_update = graph
            buf = M.ppo.RolloutBuffer(T, N, 'cuda')
            buf.obs.copy_(torch.from_numpy(src[rs.randint(0, len(src), size=n)].reshape(T, N, 780).copy()))
            buf.obs_next.copy_(torch.from_numpy(src[rs.randint(0, len(src), size=n)].reshape(T, N, 780).copy()))
            buf.act.copy_(torch.from_numpy(rs.randint(0, 15, size=(T, N)).astype(np.int32)))
            buf.done.copy_(torch.from_numpy((rs.rand(T, N) < 0.05).astype(np.uint8)))
            for it in range(3):
                buf.rew.copy_(torch.from_numpy(rs.randn(T, N).astype(np.float32)))
                buf.filled = T
                np.random.seed(it)
                res = pol.update(0, buf, is_train=True, batch_size=512, repeat=1)
            assert pol.graph_replays == (want_replays if graph else 0)
            got.append((np.array(res['loss']), pol.engine.ac.flat_p.clone()))
        np.testing.assert_allclose(got[1][0], got[0][0], rtol=2e-4, atol=2e-5)
        assert (got[1][1] - got[0][1]).abs().max().item() <= 4 * 5e-4
