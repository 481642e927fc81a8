#!/usr/bin/env python3
"""The files of the reference's Jin2022 x 4G dataset tree that its loaders read for the train / valid / test splits of the shipped PPO run,
byte for byte, as xz-compressed tar archives under tests/golden/ (each below 1 MiB):

    python tools/gen_golden_reference_tree.py <reference checkout>

  jin2022_4g_reference_tree_<k>.tar.xz   config.yml (settings only) and datasets/...: the video manifests (JSON), the viewport prediction
                                         pickles (HMDTrace format) and the 4G trace pickles of every episode in the three catalogues -- the
                                         ids listed in tests/golden/env_tables_jin2022_4g.npz.
tests/test_host_real_tables.py unpacks them and reads them with the build's loader (EnvTables.arrays_from_dataset).  Data only."""
import io
import os
import sys
import tarfile

import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import _golden  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden')
LIMIT = 1 << 20


def files_of(ref):
    cfg = yaml.safe_load(open(os.path.join(ref, 'config.yml')))
    G = _golden.load(os.path.join(OUT, 'env_tables_jin2022_4g.npz'))
    manifests, rest = set(), set()
    for sp in ('train', 'valid', 'test'):
        manifests.update(f'datasets/Jin2022/video_manifests/video{int(v)}.json' for v in G[f'{sp}/ids_v'])
        rest.update(f'datasets/Jin2022/viewports/prediction/video{int(v)}/user{int(u)}.pkl' for v, u in G[f'{sp}/ids_vp'])
        rest.update('datasets/network/4G/' + cfg['network_info']['4G'][int(t)] for t in G[f'{sp}/ids_t'])
    manifests = sorted(manifests, key=lambda p: int(p.rsplit('video', 1)[1][:-5]))
    half = len(manifests) // 2
    return [['config.yml'] + sorted(rest), manifests[:half], manifests[half:]]


def write(ref, names, path):
    buf = io.BytesIO()
    with tarfile.open(fileobj=buf, mode='w:xz', preset=9) as tar:
        for n in names:
            data = open(os.path.join(ref, n), 'rb').read()
            info = tarfile.TarInfo(n)
            info.size, info.mtime, info.mode = len(data), 0, 0o644
            tar.addfile(info, io.BytesIO(data))
    if len(buf.getvalue()) > LIMIT:
        raise SystemExit(f'{path}: {len(buf.getvalue())} bytes, more than a committed file may hold')
    open(path, 'wb').write(buf.getvalue())
    print(path, len(names), 'files', len(buf.getvalue()), 'B')


if __name__ == '__main__':
    ref = sys.argv[1]
    for k, names in enumerate(files_of(ref), 1):
        write(ref, names, os.path.join(OUT, f'jin2022_4g_reference_tree_{k}.tar.xz'))
