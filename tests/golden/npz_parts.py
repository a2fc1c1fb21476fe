"""Golden vectors kept under the 1 MiB limit of a committed file: one set of arrays is stored as several compressed parts,
<stem>.npz, <stem>.part1.npz, ...; an array larger than CHUNK bytes is flattened and cut into pieces '<name>#<i>' with its
shape under '<name>#shape'.  load_parts() puts the set back together (every lookup returns a fresh copy, as np.load does)."""
import glob
import os

import numpy as np

CHUNK = 512 << 10  # raw bytes per piece of a large array
PART = 768 << 10  # raw bytes per part file (compressed it holds at most that, plus the zip headers)


def save_parts(stem, arrays):
    for old in glob.glob(stem + ".part*.npz"):
        os.remove(old)
    pieces = []
    for name, v in arrays.items():
        a = np.asarray(v)
        if a.nbytes > CHUNK:
            flat = a.reshape(-1)
            per = max(1, CHUNK // a.itemsize)
            pieces.append((name + "#shape", np.asarray(a.shape, dtype=np.int64)))
            pieces += [(f"{name}#{i}", flat[j:j + per]) for i, j in enumerate(range(0, flat.size, per))]
        else:
            pieces.append((name, a))
    parts, cur, size = [], {}, 0
    for name, a in pieces:
        if cur and size + a.nbytes > PART:
            parts.append(cur)
            cur, size = {}, 0
        cur[name] = a
        size += a.nbytes
    parts.append(cur)
    for i, p in enumerate(parts):
        np.savez_compressed(stem + (".npz" if i == 0 else f".part{i}.npz"), **p)


class Parts(dict):
    def __getitem__(self, key):
        return dict.__getitem__(self, key).copy()


def load_parts(stem):
    files = [stem + ".npz"] + sorted(glob.glob(stem + ".part*.npz"), key=lambda p: int(p[len(stem) + 5:-4]))
    out, pieces, shapes = Parts(), {}, {}
    for f in files:
        with np.load(f, allow_pickle=True) as d:
            for k in d.files:
                if "#" not in k:
                    dict.__setitem__(out, k, d[k])
                    continue
                name, i = k.rsplit("#", 1)
                if i == "shape":
                    shapes[name] = tuple(int(x) for x in d[k])
                else:
                    pieces.setdefault(name, {})[int(i)] = d[k]
    for name, ps in pieces.items():
        dict.__setitem__(out, name, np.concatenate([ps[i] for i in sorted(ps)]).reshape(shapes[name]))
    return out
