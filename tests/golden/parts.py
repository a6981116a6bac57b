"""Golden .npz files stored in parts, so that no committed file passes 1 MiB.

save_parts("x.npz", arrays) writes x.part00.npz, x.part01.npz, ... (compressed, the arrays in their
given order, each part at most PART_BYTES) instead of x.npz; load("x.npz") reads x.npz where it
exists and the parts otherwise, as one mapping with .files like numpy's NpzFile.
"""
import glob
import io
import os

import numpy as np

PART_BYTES = 900 * 1024


def _part_paths(path):
    return sorted(glob.glob(path[:-len(".npz")] + ".part[0-9][0-9].npz"))


def save_parts(path, arrays, part_bytes=PART_BYTES):
    assert path.endswith(".npz")
    parts, size = [{}], 0
    for key, a in arrays.items():
        buf = io.BytesIO()
        np.savez_compressed(buf, **{key: a})
        n = buf.getbuffer().nbytes
        if n > part_bytes:
            raise ValueError("%s: %d bytes compressed, more than a part holds" % (key, n))
        if parts[-1] and size + n > part_bytes:
            parts.append({})
            size = 0
        parts[-1][key] = a
        size += n
    for old in _part_paths(path) + [path]:
        if os.path.exists(old):
            os.remove(old)
    for i, part in enumerate(parts):
        np.savez_compressed("%s.part%02d.npz" % (path[:-len(".npz")], i), **part)
    return len(parts)


class Parts:
    """The arrays of several .npz files under one mapping (keys in file order, read on demand)."""

    def __init__(self, paths):
        self._where, self.files = {}, []
        for p in paths:
            z = np.load(p, allow_pickle=False)
            for k in z.files:
                if k in self._where:
                    raise KeyError("%s: %s is in two parts" % (p, k))
                self._where[k] = z
                self.files.append(k)

    def __getitem__(self, key):
        return self._where[key][key]

    def __contains__(self, key):
        return key in self._where

    def __iter__(self):
        return iter(self.files)

    def __len__(self):
        return len(self.files)

    def keys(self):
        return list(self.files)


def load(path):
    if os.path.exists(path):
        return np.load(path, allow_pickle=False)
    paths = _part_paths(path)
    if not paths:
        raise FileNotFoundError(path)
    return Parts(paths)
