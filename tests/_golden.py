"""Test helper: read a fixture of tests/golden/.  Every committed file stays below 1 MiB, so a fixture too large for one file is
stored as `<name>.npz` plus `<name>.npz.part1`, `<name>.npz.part2`, ... -- more arrays of the same archive, split by key
(tools/split_golden.py).  load() reads all of them back as one read-only mapping that behaves like np.load's NpzFile: every
access returns a fresh array."""
import glob
import io
from collections.abc import Mapping

import numpy as np


def parts(path):
    """The fixture's files: `path` first, then its parts in order."""
    extra = glob.glob(glob.escape(path) + '.part*')
    return [path] + sorted(extra, key=lambda p: int(p.rsplit('.part', 1)[1]))


class Npz(Mapping):
    def __init__(self, arrays):
        self._arrays = arrays

    def __getitem__(self, key):
        return self._arrays[key].copy()

    def __iter__(self):
        return iter(self._arrays)

    def __len__(self):
        return len(self._arrays)

    @property
    def files(self):
        return list(self._arrays)

    def close(self):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


def load(path, **kw):
    """np.load(path) of a fixture archive, parts included."""
    arrays = {}
    for p in parts(path):
        with np.load(p, **kw) as z:
            for k in z.files:
                if k in arrays:
                    raise KeyError(f'{p}: array {k} is already in an earlier part')
                arrays[k] = z[k]
    return Npz(arrays)


def as_file(path):
    """The whole fixture as ONE in-memory .npz, for readers that take a file (EnvTables.from_file)."""
    buf = io.BytesIO()
    np.savez(buf, **load(path))
    buf.seek(0)
    return buf
