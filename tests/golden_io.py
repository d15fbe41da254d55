"""Golden .npz archives in parts.

No committed file may exceed 1 MiB, so an archive that would is stored as NAME.npz plus NAME.part1.npz,
NAME.part2.npz, ... with disjoint keys (save_npz_parts, used by tests/golden/make_*.py); load_npz returns the
arrays of NAME.npz and of every part beside it as one dict."""
import glob
import os

import numpy as np

LIMIT = 1 << 20


def load_npz(path):
    out = {}
    for p in [path] + sorted(glob.glob(path[:-len(".npz")] + ".part*.npz")):
        with np.load(p, allow_pickle=False) as g:
            out.update({k: g[k] for k in g.files})
    return out


def save_npz_parts(path, arrs, limit=LIMIT):
    """np.savez_compressed(path, **arrs), split greedily in key order into parts that each stay under `limit`."""
    for old in glob.glob(path[:-len(".npz")] + ".part*.npz"):
        os.remove(old)
    todo, part = list(arrs.items()), 0
    while todo:
        name = path if part == 0 else f"{path[:-len('.npz')]}.part{part}.npz"
        n = len(todo)
        while True:
            np.savez_compressed(name, **dict(todo[:n]))
            if os.path.getsize(name) <= limit or n == 1:
                break
            n -= 1
        if os.path.getsize(name) > limit:
            raise ValueError(f"{todo[0][0]} alone exceeds {limit} bytes in {name}")
        todo, part = todo[n:], part + 1
