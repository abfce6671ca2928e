"""Frames, the route's gate restated, and the references for the partition-route tests (tests/test_partition_cases_cpu.py,
tests/test_partition_route_gpu.py; the route: csrc/keyed_partition.hip).

frame(p, bias, dtype): a shuffled frame with dense int64 keys, built from the bucket shapes the accumulate kernel treats differently.
B = ids per bucket at that width (256 for p <= 8, 128 for 9 .. 12, 64 from 13: 1, 2 or 4 threads own an id's moment record).  The
smallest key is negative and sits 5 ids behind a bucket boundary, so the dense ids start in front of it.  Buckets from that boundary:

    light   n_light - 1 of them, then one more as the LAST bucket, of which only the lower half is used.  Every third id is a group
            of 3p' + 8 .. 3p' + 120 rows; every 17th group has fewer than p' rows (null; none where p' = 1); for p >= 2 every 23rd
            has column 1 = 2 x column 0 (null under the default gate)
    empty   no key falls in it: its rows of the id-indexed table are only ever written by part_zero_rows_kernel
    heavy   two keys of 4 400 .. 4 600 rows (the second and the last id of the bucket) + 12 ordinary groups: one chunk (< 32 768
            records) in which both keys pass 64 records in every tile -- the workgroup-wide heavy-id loop
    giant   one key (the last id but one) + 10 ordinary groups, 2 x 32 768 + 150 records in all: three chunks that meet in the table
            through atomics, the last shorter than a tile; the key holds > 90 % of every tile: several 256-thread rounds per tile

~1.1e5 rows (the route refuses fewer than 2^16), a key range of a few thousand ids.  Features are standard normal,
y = X beta + 1e-3 key + 0.1 noise (+ 0.5 with a bias).  The truth is report_reference.beta (extended-precision normal equations) on
the data as the device sees it: f32 frames are rounded first.
"""
import functools

import numpy as np

import report_reference as rr

F64_TOL = 1e-10  # the project's f64 parity tolerance (tests/test_gpu_parity.py)
F32_TOL = 1e-4
CHUNK = 32768        # records per accumulate workgroup (kPartAccumChunk)
HEAVY = 64           # records of one id in a tile beyond which the id is "heavy" (kHeavy)
KEY_SLOTS = 8192     # histogram slots of the order check (kKeySlots)
MAX_BUCKETS = 32768
MIN_ROWS = 1 << 16

F64_WIDTHS = tuple(range(1, 17))
F32_WIDTHS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13, 16)  # every accumulate instantiation, every f32 record size (16 .. 80 bytes)
HOST_WIDTHS = (3, 10, 16)
PRED_F32 = ((8, True), (16, True))


def bias_of(p):
    """alternating, so that p = 16 has one (p' = 17)"""
    return p % 2 == 0


def cases():
    """every (p, bias, dtype) the GPU tests use"""
    return [(p, bias_of(p), np.float64) for p in F64_WIDTHS] + [(p, bias_of(p), np.float32) for p in F32_WIDTHS]


# ------------------------------------------------------------------------------------------------- the route's layout and gate, restated
def layout(p, itemsize):
    """keyed_partition.hip make_layout: padded width, moment-record stride, threads per id, ids per bucket, record bytes, tile"""
    pc = next(s for s in (1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16) if p <= s)
    nv = (pc + 2) * (pc + 3) // 2
    tpi = 1 if nv <= 55 else (2 if nv <= 110 else 4)
    meta = ((pc + 1) * itemsize + 7) & ~7
    rs = (meta + 8 + 15) & ~15
    return dict(pc=pc, nv=nv, nvp=nv | 1, tpi=tpi, B=256 // tpi, rs=rs, tile=512 if rs <= 96 else 256)


def ids_per_bucket(p):
    return 256 if p <= 8 else (128 if p <= 12 else 64)


def gate(p, n_rows, kmin, kmax, itemsize):
    """keyed_partition_buckets + the base of lr_by_key_impl: the bucket count, or 0 where the route refuses the frame.  A restatement:
    the proof that a call took the route is pds_debug_last_by_key_route on the device."""
    if not 1 <= p <= 16 or n_rows < MIN_ROWS or n_rows >= 1 << 31:
        return 0
    L = layout(p, itemsize)
    B = L["B"]
    base = kmin - kmin % B  # (Python's %: rounded DOWN also for negative keys)
    rng_ = kmax - base + 1
    if rng_ > 1 << 31 or rng_ > 4 * n_rows:
        return 0
    nb = (rng_ + B - 1) // B
    if nb > MAX_BUCKETS:
        return 0
    table = nb * B * L["nvp"] * 8
    if table > 2 * n_rows * (p + 1) * itemsize or table > 16 << 30:
        return 0
    return nb


# ------------------------------------------------------------------------------------------------- frames
class Frame:
    """X [n, p], y [n], keys [n] (shuffled, in `dtype`); per group in ascending key order: uk, cnt, null (constructed), small, collinear,
    kind ("light" / "heavy" / "giant": the bucket's), big (the heavy and giant KEYS); buckets: name -> bucket index (light: a list)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def n_groups(self):
        return len(self.uk)

    @functools.cached_property
    def order(self):
        return np.argsort(self.keys, kind="stable")

    @functools.cached_property
    def off(self):
        return np.concatenate([[0], np.cumsum(self.cnt)]).astype(np.int64)

    def group(self, g):
        """group g's rows as f64 (design with the bias column appended, y)"""
        rows = self.order[self.off[g]: self.off[g + 1]]
        X = self.X[rows].astype(np.float64)
        return (np.column_stack([X, np.ones(len(X))]) if self.bias else X), self.y[rows].astype(np.float64)

    def bucket_sizes(self):
        nb = int((self.uk[-1] - self.base) // self.B) + 1
        return np.bincount((self.uk - self.base) // self.B, weights=self.cnt, minlength=nb).astype(np.int64)


N_LIGHT = {256: 4, 128: 6, 64: 10}  # (fewer ids per bucket: more light buckets, so that the nulls of every 17th / 23rd group exist)


@functools.lru_cache(maxsize=6)
def frame(p, bias, dtype=np.float64):
    dtype = np.dtype(dtype).type
    bias = bool(bias)
    rng = np.random.default_rng(52_000 + 100 * p + 10 * int(bias) + (1 if dtype is np.float32 else 0))
    pp = p + int(bias)
    B = ids_per_bucket(p)
    nl = N_LIGHT[B]
    base = -2 * B
    first = base + 5
    b_light = list(range(nl - 1)) + [nl + 2]
    b_empty, b_heavy, b_giant = nl - 1, nl, nl + 1

    ids, sizes, kinds, big = [], [], [], []
    lo_, hi_ = 3 * pp + 8, 3 * pp + 120

    def ordinary(k):
        return rng.integers(lo_, hi_ + 1, size=k)

    def add(bucket, local, size, big_=None):
        for l, s in zip(np.atleast_1d(local), np.atleast_1d(size)):
            ids.append(bucket * B + int(l))
            sizes.append(int(s))
            kinds.append("light" if bucket in b_light else ("heavy" if bucket == b_heavy else "giant"))
            big.append(bool(big_))

    for b in range(nl + 3):
        if b in b_light:
            loc = np.array([l for l in range(B if b != nl + 2 else B // 2) if (b * B + l) % 3 == 2 and b * B + l >= 5])
            add(b, loc, ordinary(len(loc)))
        elif b == b_heavy:
            add(b, 1, rng.integers(4400, 4601), True)
            add(b, 4 + 3 * np.arange(12), ordinary(12))
            add(b, B - 1, rng.integers(4400, 4601), True)
        elif b == b_giant:
            o = ordinary(10)
            add(b, 3 + 5 * np.arange(10), o)
            add(b, B - 2, 2 * CHUNK + 150 - int(o.sum()), True)
    ids, sizes, kinds, big = np.array(ids), np.array(sizes), np.array(kinds), np.array(big)
    assert np.all(np.diff(ids) > 0)
    G = len(ids)
    light = np.flatnonzero(kinds == "light")
    small = np.zeros(G, dtype=bool)
    collinear = np.zeros(G, dtype=bool)
    if pp > 1:
        small[light[16::17]] = True
        sizes[small] = rng.integers(1, pp, size=int(small.sum()))
    if p >= 2:
        collinear[light[11::23]] = True
        collinear &= ~small
    off = np.concatenate([[0], np.cumsum(sizes)])
    N = int(off[-1])
    key = np.repeat(ids + base, sizes).astype(np.int64)
    X = rng.normal(size=(N, p))
    for g in np.flatnonzero(collinear):
        X[off[g]: off[g + 1], 1] = 2.0 * X[off[g]: off[g + 1], 0]
    y = X @ rng.normal(size=p) + 1e-3 * key + 0.1 * rng.normal(size=N) + (0.5 if bias else 0.0)
    perm = rng.permutation(N)
    f = Frame(p=p, bias=bias, pp=pp, dtype=dtype, B=B, base=base, X=np.ascontiguousarray(X[perm].astype(dtype)),
              y=np.ascontiguousarray(y[perm].astype(dtype)), keys=np.ascontiguousarray(key[perm]), uk=ids + base, cnt=sizes,
              null=small | collinear, small=small, collinear=collinear, kind=kinds, big=big,
              buckets=dict(light=b_light, empty=b_empty, heavy=b_heavy, giant=b_giant))
    assert int(f.keys.min()) == first
    for a in (f.X, f.y, f.keys, f.uk, f.cnt, f.null):
        a.setflags(write=False)
    return f


# ------------------------------------------------------------------------------------------------- references
_TRUTH = {}


def truth(f):
    """report_reference.beta on every constructed non-null group: [G, p'], NaN rows for the null groups.  Computed once per frame."""
    k = (f.p, f.bias, f.dtype)
    if k not in _TRUTH:
        t = np.full((f.n_groups, f.pp), np.nan)
        for g in np.flatnonzero(~f.null):
            t[g] = rr.beta(*f.group(g))
        t.setflags(write=False)
        _TRUTH[k] = t
    return _TRUTH[k]


def oracle_by(orc, f):
    """the f64 oracle's per-group fit (orc.pl_lr, default gate) on every group with at least p' rows: (coeffs [G, p'], null [G])"""
    co = np.full((f.n_groups, f.pp), np.nan)
    nu = np.ones(f.n_groups, dtype=bool)
    for g in np.flatnonzero(f.cnt >= f.pp):
        A, y = f.group(g)
        b = orc.pl_lr(A[:, :f.p], y, add_bias=f.bias)
        if b is not None:
            co[g], nu[g] = b, False
    return co, nu


def nrel_rows(a, t):
    """normwise relative distance per row: ||a_g - t_g|| / ||t_g||"""
    a, t = np.asarray(a, np.float64), np.asarray(t, np.float64)
    return np.linalg.norm(a - t, axis=1) / np.maximum(np.linalg.norm(t, axis=1), 1e-300)


# ------------------------------------------------------------------------------------------------- more buckets than histogram slots
BIG_BUCKETS = 16_600
BIG_ROWS = 7_700_000


@functools.lru_cache(maxsize=1)
def big_frame():
    """p = 1, no bias, f64: keys random over 16 600 x 256 ids, x in {1, 2, 3}, y an integer in -4 .. 4 -- every moment is an exact
    integer whatever the order of the sums.  Returns (x, y, keys, uk, beta_ref) with beta_ref = Sxy / Sxx from np.bincount (exact
    integer sums, one correctly rounded division)."""
    rng = np.random.default_rng(16_600)
    n_ids = BIG_BUCKETS * 256
    keys = rng.integers(0, n_ids, size=BIG_ROWS, dtype=np.int64) - 1000
    keys[:2] = (-1000, n_ids - 1001)  # (the whole range is used)
    x = rng.integers(1, 4, size=BIG_ROWS).astype(np.float64)
    y = rng.integers(-4, 5, size=BIG_ROWS).astype(np.float64)
    dense = keys + 1000
    sxx = np.bincount(dense, weights=x * x, minlength=n_ids)
    sxy = np.bincount(dense, weights=x * y, minlength=n_ids)
    used = np.flatnonzero(sxx > 0)
    assert sxx.max() < 2 ** 53 and np.abs(sxy).max() < 2 ** 53
    for a in (x, y, keys):
        a.setflags(write=False)
    return x, y, keys, used - 1000, sxy[used] / sxx[used]
