"""The Goldilocks leaf hash and Merkle tree layout stated a second time, from the reference comments at the top of csrc/merkle.hip
(linearhash.js:22-41, linearhash_gpu.js:30-66, merklehash_p.js:28-103) and sharing with the C oracle nothing but its permutation
(gl_oracle.poseidon, which takes any 64-bit words and hashes their residues).  Beside the checker: the shapes that
tests/test_merkle_ref_cpu.py and tests/test_gpu_merkle_edges.py both run, and the generator of words at or above p."""
import numpy as np

P = 0xFFFFFFFF00000001
TOP = (1 << 64) - 1

# every width at which the leaf kernels are compared row by row: nothing, the passthrough widths (<= 4), one chunk (5..8), then for the
# split form every (batch count, class of the last batch) that exists -- test_merkle_ref_cpu.py enumerates them from split_shape()
WIDTHS = [0, 1, 3, 4, 5, 7, 8, 9, 12, 13, 16, 17, 20, 21, 24, 25, 28, 29, 32, 33, 35, 37, 45, 49, 100, 113]
HEIGHT_EVERY_WIDTH = 513                   # two plain workgroups (256 rows) and a row; one split workgroup (512 rows) and a row
HEIGHT_WIDTHS = [3, 9, 33, 100]            # passthrough, two batches with a 1-column last one, four one-chunk.., four several-chunk batches
HEIGHTS = [1, 63, 64, 65, 255, 256, 257, 511, 512, 1025]      # the wave (64), plain workgroup (256) and split workgroup (512) edges
# whole trees: 12 and 1028 have their first odd level at depth 2 (3 and 257 digests), 258 and 2^13 + 2 at depth 1; 4097 is odd at every
# depth down to the level of three digests
TREE_HEIGHTS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 15, 16, 17, 31, 33, 63, 64, 65, 255, 256, 257, 258, 511, 513, 1000, 1028, 4095, 4096, 4097,
                (1 << 13) + 2]
REF_TREE_MAX = 1 << 10                     # tree() is Python over one permutation call per node: only up to here


def leaf_shapes():
    """(width, height) of every leaf comparison"""
    return [(w, HEIGHT_EVERY_WIDTH) for w in WIDTHS] + [(w, h) for w in HEIGHT_WIDTHS for h in HEIGHTS]


def _poseidon(inp, cap):
    import gl_oracle
    return [int(v) for v in gl_oracle.poseidon(np.array(inp, dtype=np.uint64), None if cap is None else np.array(cap, dtype=np.uint64), 4)]


def _plain(v):
    """linearhash.js:22-41: up to four words are their own digest, zero-padded; otherwise the sponge over chunks of 8, capacity 0 first"""
    v = [int(x) for x in v]
    if len(v) <= 4:
        return v + [0] * (4 - len(v))
    st = [0, 0, 0, 0]
    for i in range(0, len(v), 8):
        c = v[i:i + 8]
        st = _poseidon(c + [0] * (8 - len(c)), st)
    return st


def split_batch(w):
    return max(8, (w + 3) // 4)


def leaf(row, split):
    """the digest (4 ints) of one row; split (linearhash_gpu.js:30-66), for widths above 8: batches of max(8, ceil(w / 4)) columns, each
    hashed plainly, then the digests side by side hashed plainly"""
    row = [int(x) for x in row]
    if not split or len(row) <= 8:
        return _plain(row)
    b = split_batch(len(row))
    side = []
    for i in range(0, len(row), b):
        side += _plain(row[i:i + b])
    return _plain(side)


DIGEST, ONE_CHUNK, CHUNKS = "own digest", "one chunk", "several chunks"


def split_shape(w):
    """(batch count, class of the last batch) of the split form at width w"""
    b = split_batch(w)
    nb = max(1, (w + b - 1) // b)
    last = w - (nb - 1) * b
    return nb, (DIGEST if last <= 4 else ONE_CHUNK if last <= 8 else CHUNKS)


def level_sizes(height):
    """digests per level, leaves first, root (1) last; a 1-row tree has the leaf level alone"""
    s = [height]
    while s[-1] > 1:
        s.append((s[-1] + 1) // 2)
    return s


def num_nodes(height):
    """words of the node array (merklehash_p.js:28-42): every level but the root padded to an even count of digests, then the root's four
    words.  The 1-row quirk: the loop that would copy nothing still reserves a padded leaf level, 8 words, and the last four stay zero"""
    s = level_sizes(height)
    if len(s) == 1:
        return 8
    return sum(4 * (n + (n & 1)) for n in s[:-1]) + 4


def tree(rows, split):
    """the node array of the tree over `rows` (height x width), as uint64"""
    rows = np.asarray(rows)
    h = rows.shape[0]
    nodes = [0] * num_nodes(h)
    level = [leaf(r, split) for r in rows]
    off = 0
    while True:
        for i, d in enumerate(level):
            nodes[off + 4 * i:off + 4 * i + 4] = d
        if len(level) == 1:
            break
        if len(level) & 1:
            level = level + [[0, 0, 0, 0]]                # an odd level is padded with a zero digest
        off += 4 * len(level)
        level = [_poseidon(level[2 * i] + level[2 * i + 1], None) for i in range(len(level) // 2)]
    return np.array(nodes, dtype=np.uint64)


def full_range(rng, shape):
    """uniform words below p (both 32-bit halves busy)"""
    a = rng.integers(0, 1 << 63, size=shape, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=shape, dtype=np.uint64)
    return np.where(a >= np.uint64(P), a - np.uint64(P), a).astype(np.uint64)


def noncanonical(rng, shape, cols=None):
    """full-range words of which about a third are at or above p (p .. 2^64 - 1: 2^32 - 1 values), with p, p + 1 and 2^64 - 1 forced in.
    cols: the columns (last axis) that take such words; the others stay below p"""
    a = full_range(rng, shape)
    if a.size == 0:
        return a
    high = np.uint64(P) + rng.integers(0, TOP - P + 1, size=shape, dtype=np.uint64)
    pick = rng.random(shape) < 1 / 3
    ok = np.zeros(shape, bool)
    if cols is None:
        ok[...] = True
    else:
        ok[..., sorted(set(cols))] = True
    a = np.where(pick & ok, high, a)
    where = np.flatnonzero(ok.reshape(-1))
    flat = a.reshape(-1)
    spots = rng.choice(where, size=min(3, where.size), replace=False)
    for s, v in zip(spots, (TOP, P, P + 1)):
        flat[s] = v
    return flat.reshape(shape)


def residues(a):
    a = np.asarray(a, dtype=np.uint64)
    return np.where(a >= np.uint64(P), a - np.uint64(P), a)


def noncanonical_columns(w, split):
    """the columns of a width-w row where words at or above p matter most: every column of a passthrough width; otherwise the first chunk
    of every batch, the ragged last chunk of every batch, and a last batch of at most 4 columns whole"""
    if w <= 4:
        return list(range(w))
    b = split_batch(w) if split and w > 8 else max(w, 1)
    cols = set()
    for s in range(0, w, b):
        e = min(s + b, w)
        cols.update(range(s, min(s + 8, e)))              # the first chunk (a batch of <= 4 columns is all here)
        cols.update(range(s + (e - s - 1) // 8 * 8, e))   # the last chunk, ragged or not
    return sorted(cols)
