"""CPU: the packed Jin2022 x 4G table fixture (tests/golden/env_tables_jin2022_4g.npz, written by tools/gen_golden_tables_full.py out of the
reference's own loaders) against the build's host-side loader and catalogue logic, and the known answers the reference's shipped run holds
for host logic: the minibatch split behind `save/gradient_step` = 18 and the catalogue walk behind the order of train_log.csv / valid_log.csv."""
import glob
import os
import tarfile

import numpy as np
import pytest

import _jin2022_tree as jt
from mansy_immersivevideostreaming_amd.bitrate_selection.envs.mansy_env import (EnvTables, generate_environment_samples,
                                                                                generate_environment_test_samples)
from mansy_immersivevideostreaming_amd.bitrate_selection.models.mansy_ppo import split_indices
from mansy_immersivevideostreaming_amd.bitrate_selection.utils.common import get_config_from_yml

G = jt.load()


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('jin2022_host'))
    return root, jt.make_tree(root, G)


def test_fixture_shapes_and_catalogues():
    assert G['train/samples'].shape == (72, 4) and G['valid/samples'].shape == (48, 4) and G['test/samples'].shape == (1440, 4)
    for sp in jt.SPLITS:
        v, u, t = (list(G[f'{sp}/list_{k}']) for k in ('videos', 'users', 'traces'))
        qw = G[f'{sp}/qoe_w']
        cat = generate_environment_test_samples(v, u, t, qw) if sp == 'test' else generate_environment_samples(v, u, t, qw, seed=5)
        ids = np.array([(v[a], u[b], t[c]) for a, b, c, _ in cat])
        assert np.array_equal(ids, G[f'{sp}/ids_samples']) and [c[3] for c in cat] == G[f'{sp}/samples'][:, 3].tolist()
    # the shipped results.csv IS the exhaustive test enumeration (utils/common.py:87-98), preference fastest
    assert np.array_equal(G['shipped/results_ids'], G['test/ids_samples'])
    assert np.array_equal(G['shipped/results_w'], G['test/qoe_w'][G['test/samples'][:, 3]])


def test_tree_written_from_the_fixture_loads_back_bit_identical(tree):
    """`EnvTables.arrays_from_dataset` (the host half of from_dataset: what Simulator.__init__ reads, simulator.py:30-45) over the dataset
    tree the GPU tests materialise == the arrays the reference's loaders produced."""
    root, cfg = tree
    config = get_config_from_yml(cfg)
    for sp in jt.SPLITS:
        arrays, ids = EnvTables.arrays_from_dataset(config, 'Jin2022', '4G', sp, config.qoe_split['train'], seed=5)
        for k in EnvTables.FIELDS:
            assert arrays[k].dtype == G[f'{sp}/{k}'].dtype and np.array_equal(arrays[k], G[f'{sp}/{k}']), (sp, k)
        assert np.array_equal(np.array(ids[3]), G[f'{sp}/ids_samples'])


@pytest.fixture(scope='module')
def reference_tree(tmp_path_factory):
    """The reference's own dataset files for the three catalogues, byte for byte (tests/golden/jin2022_4g_reference_tree_*.tar.xz,
    tools/gen_golden_reference_tree.py), unpacked in the reference's layout: config.yml next to datasets/ and bitrate_selection/."""
    root = str(tmp_path_factory.mktemp('jin2022_reference'))
    archives = sorted(glob.glob(os.path.join(os.path.dirname(__file__), 'golden', 'jin2022_4g_reference_tree_*.tar.xz')))
    assert len(archives) == 3, archives
    for a in archives:
        with tarfile.open(a) as tar:
            tar.extractall(root, filter='data')
    os.makedirs(os.path.join(root, 'bitrate_selection'))
    return root


def test_loader_on_the_reference_tree_equals_the_reference_loaders(reference_tree):
    cwd = os.getcwd()
    os.chdir(os.path.join(reference_tree, 'bitrate_selection'))           # config.yml's directories are relative to the reference's scripts
    try:
        config = get_config_from_yml(os.path.join(reference_tree, 'config.yml'))
        for sp in jt.SPLITS:
            arrays, ids = EnvTables.arrays_from_dataset(config, 'Jin2022', '4G', sp, config.qoe_split['train'], seed=5)
            for k in EnvTables.FIELDS:
                assert np.array_equal(arrays[k], G[f'{sp}/{k}']), (sp, k)
    finally:
        os.chdir(cwd)


def test_gradient_step_18_pins_the_merge_last_split():
    """Shipped tfevents: save/gradient_step = 18 at save/env_step = 6000 with step-per-collect 2000, batch 512, repeat 2: three collects x two
    passes x THREE minibatches.  Batch.split(512, merge_last=True) over 2000 rows gives 512 / 512 / 976; without merge_last it would be four
    (gradient_step 24).  tianshou counts a collect's gradient steps as len(losses['loss'])."""
    assert G['shipped/tb/save/gradient_step'][0, 1] == 18 and G['shipped/tb/save/env_step'][0, 1] == 6000
    chunks = [len(c) for c in split_indices(2000, 512)]
    assert chunks == [512, 512, 976]
    assert 3 * 2 * len(chunks) == 18
    assert [len(c) for c in split_indices(2000, 512, merge_last=False)] == [512, 512, 512, 464]
    assert sorted(np.concatenate(list(split_indices(2000, 512))).tolist()) == list(range(2000))


def _walk(worker_id, worker_num, n_sample):
    """MANSYEnv.reset's catalogue walk (mansy_env.py:100-101): returns the entry, advances by worker_num."""
    while True:
        yield worker_id % n_sample
        worker_id = (worker_id + worker_num) % n_sample


def _row_entry(ids, w, split):
    cat_ids, cat_q, qw = G[f'{split}/ids_samples'], G[f'{split}/samples'][:, 3], G[f'{split}/qoe_w']
    hit = [i for i in range(len(cat_ids)) if (cat_ids[i] == ids).all() and (qw[cat_q[i]] == w).all()]
    assert len(hit) == 1
    return hit[0]


def test_shipped_logs_follow_the_catalogue_walk_with_tianshous_resets():
    """train_log.csv: ONE training environment (run_mansy.py:37 forces train_num 1), seed 5 % 1 = worker 0, entries 0, 1, 2, ... in order --
    119 finished episodes in 6000 steps = 39 + 40 + 40 (tfevents train/episode), lengths from the tables (49 / 51 / 37 .. chunk videos).
    valid_log.csv: four workers with seeds 5..8 (DummyVectorEnv.seed: seed + i -> worker_id 1, 2, 3, 0), 48 episodes per test = 12 lock-step
    rounds, rows in worker order; before a test's first episode every worker has been reset once by Collector.__init__ and once by
    test_episode's reset_env, after its 12 episodes once per episode end and once more by collect()'s closing reset_env: the first test
    starts at entries 5, 6, 7, 4, the second at 13, 14, 15, 12."""
    tr = [_row_entry(G['shipped/train_log_ids'][i], G['shipped/train_log_w'][i], 'train') for i in range(119)]
    assert tr == [i % 72 for i in range(119)]
    lens = G['train/episode_len']
    steps, n_ep, ep_len_sum, per_collect = 0, 0, 0, []
    left = int(lens[0])
    entry = 0
    for collect in range(3):
        n_ep, ep_len_sum = 0, 0
        for _ in range(2000):
            left -= 1
            if left == 0:
                n_ep += 1
                ep_len_sum += int(lens[entry % 72])
                entry += 1
                left = int(lens[entry % 72])
        per_collect.append((n_ep, ep_len_sum / n_ep))
    assert [p[0] for p in per_collect] == G['shipped/tb/train/episode'][:, 1].tolist() == [39, 40, 40]
    np.testing.assert_allclose([p[1] for p in per_collect], G['shipped/tb/train/length'][:, 1], rtol=1e-6)
    va = [_row_entry(G['shipped/valid_log_ids'][i], G['shipped/valid_log_w'][i], 'valid') for i in range(96)]
    walks = [_walk((5 + i) % 4, 4, 48) for i in range(4)]
    for w in walks:
        next(w)                                     # Collector.__init__ -> reset_env
    expect = []
    for test in range(2):
        cur = [next(w) for w in walks]              # test_episode: collector.reset_env()
        for rnd in range(12):
            expect += cur                           # the four episodes end on the same step; rows in worker order
            cur = [next(w) for w in walks]          # finished environments are reset
        for w in walks:
            next(w)                                 # collect(n_episode=...) ends in reset_env()
        # (the `cur` drawn after round 12 is the per-episode reset; the closing reset_env skips one more entry)
    assert va == expect
    assert va[:4] == [5, 6, 7, 4] and va[48:52] == [13, 14, 15, 12]
