"""CPU reference of the class objects, written from the group comment "class objects" of include/tsdf_amd.h alone: labelled voxels
(rule 1), the list (rule 2), objects and their rows (rule 3) and the lookup (rule 4) in numpy and plain Python, the lookup's index
arithmetic in float32 scalars, every operation rounded on its own.  No union-find: labels spread along the graph's edges until they
stand still.  tests/test_objects_host.py checks it against cases worked out by hand."""
import numpy as np

F32 = np.float32
NONE = 0xFFFFFFFF
OBJECT_DTYPE = np.dtype([("label", np.uint32), ("size", np.uint32), ("lo", np.uint32, 3), ("hi", np.uint32, 3), ("sum", np.uint64, 3),
                         ("votes", np.uint64), ("class_id", np.uint32), ("reserved", np.uint32)])


def words_of(classes, votes):
    """The class words (class in bits 0-15, votes in bits 16-31) of per-voxel classes and votes."""
    return (np.asarray(classes, np.uint32) & np.uint32(0xFFFF)) | (np.asarray(votes, np.uint32) << np.uint32(16))


def labelled(words, min_votes=1, select=None):
    """Rules 1 - 2: the ascending ids (uint32) of the labelled voxels.  select: None, or a sequence of bytes indexed by class."""
    w = np.asarray(words, np.uint32).reshape(-1)
    c, n = (w & np.uint32(0xFFFF)).astype(np.int64), (w >> np.uint32(16)).astype(np.int64)
    keep = n >= max(int(min_votes), 1)
    if select is not None:
        s = np.asarray(select, np.uint8).reshape(-1)
        admitted = np.zeros(65536, bool)
        admitted[:len(s)] = s != 0
        keep &= admitted[c]
    return np.flatnonzero(keep).astype(np.uint32)


def coordinates(ids, size):
    X, Y, _ = size
    ids = np.asarray(ids, np.int64)
    return np.stack([ids % X, (ids // X) % Y, ids // (X * Y)], axis=1)


def objects(words, ids, size, connectivity, min_size):
    """Rule 3: (L (uint32 per listed voxel), rows (OBJECT_DTYPE, size >= min_size, ascending label), n_objects)."""
    assert connectivity in (6, 26)
    X, Y, Z = size
    w = np.asarray(words, np.uint32).reshape(-1)
    n = len(ids)
    c = coordinates(ids, size)
    cls =(w[np.asarray(ids, np.int64)] & np.uint32(0xFFFF)).astype(np.int64)
    votes = (w[np.asarray(ids, np.int64)] >> np.uint32(16)).astype(np.int64)
    # the graph's edges as pairs of list indices: one half of the neighbourhood is enough, an edge has two ends
    steps = [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
             if (dz, dy, dx) > (0, 0, 0) and (connectivity == 26 or abs(dx) + abs(dy) + abs(dz) == 1)]
    at = np.full(X * Y * Z, -1, np.int64)
    at[np.asarray(ids, np.int64)] = np.arange(n)
    at = at.reshape(Z, Y, X)
    part = lambda d, m: (slice(max(0, -d), m - max(0, d)), slice(max(0, d), m - max(0, -d)))   # (here, there) along one axis
    ends_a, ends_b = [], []
    for dx, dy, dz in steps:
        (za, zb), (ya, yb), (xa, xb) = part(dz, Z), part(dy, Y), part(dx, X)
        a, b = at[za, ya, xa].reshape(-1), at[zb, yb, xb].reshape(-1)
        both = (a >= 0) & (b >= 0)
        a, b = a[both], b[both]
        same = cls[a] == cls[b]
        ends_a.append(a[same])
        ends_b.append(b[same])
    a, b = np.concatenate(ends_a), np.concatenate(ends_b)
    # every voxel takes the smallest label among itself and its neighbours until nothing changes: the object's smallest list index
    labels = np.arange(n, dtype=np.int64)
    while True:
        low = np.minimum(labels[a], labels[b])
        new = labels.copy()
        np.minimum.at(new, a, low)
        np.minimum.at(new, b, low)
        new = new[new]                             # (a label is a member of the same object: its label is no larger)
        if np.array_equal(new, labels):
            break
        labels = new
    order = np.argsort(labels, kind="stable")
    roots, starts = np.unique(labels[order], return_index=True)
    rows = []
    for r, a, b in zip(roots, starts, list(starts[1:]) + [n]):
        member = order[a:b]
        if len(member) >= min_size:
            m = c[member]
            rows.append((r, len(member), m.min(axis=0), m.max(axis=0), m.sum(axis=0), votes[member].sum(), cls[r], 0))
    out = np.zeros(len(rows), OBJECT_DTYPE)
    for k, row in enumerate(rows):
        out[k] = row
    return labels.astype(np.uint32), out, len(roots)


def find(words, size, min_votes=1, select=None, connectivity=26, min_size=1):
    """Rules 1 - 3 in one: (ids, L, rows, n_objects)."""
    ids = labelled(words, min_votes, select)
    L, rows, n_objects = objects(words, ids, size, connectivity, min_size)
    return ids, L, rows, n_objects


def voxel_of(point, size, voxel_size, offset, offset_at_clear):
    """The voxel id the class sampler reads for a world point (rule 4; "class fusion", Sampling), or None: per axis
    i = (int)floorf(((p - offset) - offset_at_clear) / voxel_size), None for a NaN coordinate or an off-grid index."""
    i = []
    with np.errstate(all="ignore"):
        for k in range(3):
            f = np.floor(F32(F32(F32(F32(point[k]) - F32(offset[k])) - F32(offset_at_clear[k])) / F32(voxel_size[k])))
            if not (f >= 0 and f < size[k]):   # (false for NaN)
                return None
            i.append(int(f))
    return (i[2] * size[1] + i[1]) * size[0] + i[0]


def lookup(points, ids, L, rows, size, voxel_size, offset, offset_at_clear):
    """Rule 4: (n,) uint32 table rows, NONE where the point lies in no listed object."""
    index = {int(v): i for i, v in enumerate(ids)}
    row_of = {int(label): k for k, label in enumerate(rows["label"])}
    p = np.asarray(points, F32).reshape(-1, 3)
    out = np.full(len(p), NONE, np.uint32)
    for k in range(len(p)):
        v = voxel_of(p[k], size, voxel_size, offset, offset_at_clear)
        if v is None or v not in index:
            continue
        out[k] = row_of.get(int(L[index[v]]), NONE)
    return out


def random_words(size, seed, density, n_classes):
    """Class words: a share `density` of the voxels has votes drawn from {1, 2, 65535}, the rest 0 -- and half of those keep class bits,
    which rule 1 says count for nothing; classes uniform in 0 .. n_classes - 1."""
    n = size[0] * size[1] * size[2]
    rng = np.random.default_rng(seed)
    classes = rng.integers(0, n_classes, n)
    votes = np.where(rng.random(n) < density, rng.choice(np.array([1, 2, 65535]), n), 0)
    classes = np.where((votes == 0) & (rng.random(n) < 0.5), 0, classes)
    return words_of(classes, votes)
