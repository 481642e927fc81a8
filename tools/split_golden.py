#!/usr/bin/env python3
"""Keeps every fixture under tests/golden/ below 1 MiB a file: an .npz archive larger than that is rewritten as `<name>.npz` plus
`<name>.npz.part1`, `<name>.npz.part2`, ... (compressed archives holding disjoint sets of its arrays, in the archive's key order).
tests/_golden.py reads them back as one.  Run it after any gen_golden_*.py that writes a large archive; the generators rewrite `<name>.npz`
whole, and this removes the parts of the fixture's earlier version before it splits the new one:

    python tools/split_golden.py [archive.npz ...]        (default: every tests/golden/*.npz)
"""
import glob
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 1 << 20
BUDGET = 960_000          # compressed bytes per part (the zip directory and headers stay inside the limit)


def _compressed_size(arrays):
    buf = io.BytesIO()
    np.savez_compressed(buf, **arrays)
    return len(buf.getvalue())


def split(path):
    """Split `path` if it is larger than LIMIT.  Parts left from an earlier version of the fixture are removed first: a generator
    rewrites `<name>.npz` whole, so an archive that holds any array of its parts is the new whole and the parts are stale.  An archive
    whose parts hold only arrays it does not have is already split and stays as it is."""
    old = sorted(glob.glob(glob.escape(path) + '.part*'))
    with np.load(path) as z:
        arrays = {k: z[k] for k in z.files}
    if old:
        stale = False
        for p in old:
            with np.load(p) as z:
                stale = stale or bool(set(z.files) & set(arrays))
        if not stale:
            return [path] + old
        for p in old:
            os.remove(p)
            print('removed stale part', p)
    if os.path.getsize(path) <= LIMIT:
        return [path]
    groups, cur = [], {}
    for k, a in arrays.items():
        if cur and _compressed_size(dict(cur, **{k: a})) > BUDGET:
            groups.append(cur)
            cur = {}
        cur[k] = a
    groups.append(cur)
    out = []
    for i, g in enumerate(groups):
        p = path if i == 0 else f'{path}.part{i}'
        with open(p, 'wb') as fh:
            np.savez_compressed(fh, **g)
        if os.path.getsize(p) > LIMIT:
            raise SystemExit(f'{p}: {os.path.getsize(p)} bytes -- one array alone is too large for a file')
        out.append(p)
    return out


if __name__ == '__main__':
    paths = sys.argv[1:] or sorted(glob.glob(os.path.join(ROOT, 'tests', 'golden', '*.npz')))
    for p in paths:
        parts = split(p)
        if len(parts) > 1:
            print(p, '->', len(parts), 'files:', ', '.join('%s %d B' % (os.path.basename(q), os.path.getsize(q)) for q in parts))
