"""The partition route (csrc/keyed_partition.hip: histogram -> scatter -> accumulate -> compact -> solve) on the MI355X at every width,
both frame types and every bucket shape, against extended-precision normal equations (report_reference.beta).

Frames: tests/partition_cases.py -- ~1.1e5 shuffled rows with dense negative-to-positive keys: light buckets with too-small and
collinear (null) groups, an empty bucket, a one-chunk bucket with two heavy keys, a three-chunk bucket with one giant key; their
conditions and the reference alone are checked in tests/test_partition_cases_cpu.py.  Every call here first proves its route through
pds_debug_last_by_key_route (1 = partition; the bucket width and count the gate's restatement expects).

Bounds: F64_TOL = 1e-10 normwise per group on f64 frames, F32_TOL = 1e-4 on f32 frames, no group excepted (the f64 oracle is within
2.4e-15 of the truth on every compared group of these frames).

Measured on the MI355X, worst normwise distance to the truth over the non-null groups of the light buckets / the heavy bucket / the
giant bucket (the records of a bucket arrive in the order of the scatter's atomics: the last digit changes from run to run):

  f64   p   light    heavy    giant        p   light    heavy    giant
        1  1.4e-15  6.5e-16  7.6e-16       9  1.5e-15  9.6e-16  5.3e-16
        2  1.1e-15  6.8e-16  4.8e-16      10  1.6e-15  1.3e-15  6.7e-16
        3  1.2e-15  1.4e-15  4.2e-16      11  1.2e-15  1.2e-15  7.5e-16
        4  1.0e-15  1.0e-15  5.3e-16      12  1.5e-15  9.1e-16  7.0e-16
        5  1.2e-15  8.0e-16  5.6e-16      13  1.4e-15  1.0e-15  8.7e-16
        6  1.8e-15  8.4e-16  6.4e-16      14  1.6e-15  1.1e-15  8.0e-16
        7  1.4e-15  9.1e-16  6.7e-16      15  1.6e-15  1.1e-15  8.1e-16
        8  1.4e-15  8.4e-16  7.4e-16      16  1.4e-15  1.0e-15  1.2e-15
        the three big keys alone: 3.2e-16 .. 1.0e-15 -- one lost record of the giant key would move its beta by about 1e-6
  f32   p   light    heavy    giant        p   light    heavy    giant
        1  5.5e-08  5.2e-08  4.1e-08       7  4.2e-08  3.2e-08  3.5e-08
        2  4.6e-08  5.2e-08  4.4e-08       8  4.0e-08  3.7e-08  3.5e-08
        3  5.2e-08  4.2e-08  3.2e-08       9  3.7e-08  3.5e-08  2.8e-08
        4  5.3e-08  3.7e-08  4.5e-08      12  3.5e-08  3.2e-08  3.8e-08
        5  4.5e-08  4.0e-08  3.6e-08      13  3.6e-08  2.8e-08  3.3e-08
        6  4.0e-08  3.9e-08  3.5e-08      16  1.0e-07  8.2e-08  8.9e-08
        (the rounding of the f32 coefficients themselves: the moments are summed in f64)
  predictions: f64 |pred - x . beta| <= 1.4e-15 of ||x|| ||beta|| at every width, resid = y - pred bit for bit; f32 5.1e-08 (p = 8)
  and 3.9e-08 (p = 16).  The 16 601-bucket frame: 3 555 409 groups, the worst coefficient 0.98 eps from Sxy / Sxx.

What the tests notice, tried once with three deliberately wrong (memory-safe) builds of keyed_partition.hip: the heavy-id hand-over
reading scratch[e] for scratch[part * EPT + e] fails every case with p >= 9 and none below (one thread per id there); a
part_zero_rows_kernel that leaves buckets without records alone fails 39 of the 47 cases (phantom groups from stale workspace: the
first frames of a process meet a clean one); the last chunk of a three-chunk bucket dropping its last record fails all sixteen f64
widths and one f32 layout, as test_every_layout_f32 says of itself.
"""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import partition_cases as pc  # noqa: E402

pytestmark = pytest.mark.gpu

F32_EPS = float(np.finfo(np.float32).eps)


@pytest.fixture(scope="module")
def pds():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import polars_ds_extension_amd as m

    return m


def dev(a):
    import torch

    return torch.from_numpy(np.array(a, order="C")).cuda()  # (a copy: the shared frames are read-only)


def np_(v):
    return v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)


def cols_of(X, space="device"):
    cs = [np.ascontiguousarray(X[:, j]) for j in range(X.shape[1])]
    return [dev(c) for c in cs] if space == "device" else cs


def last_route():
    """(route, [part_shift, n_buckets, histogram from the order check's slots, per-row prediction mode]) of this thread's last call"""
    from polars_ds_extension_amd import _lib

    fn = _lib.load().pds_debug_last_by_key_route
    fn.restype, fn.argtypes = C.c_int, [C.POINTER(C.c_int)]
    info = (C.c_int * 4)()
    return int(fn(info)), [int(v) for v in info]


class typed:
    """the package fits in the type its configuration names"""

    def __init__(self, pds, dtype):
        self.pds, self.f64 = pds, np.dtype(dtype) == np.float64

    def __enter__(self):
        self.pds.config.LIN_REG_EXPR_F64 = self.f64

    def __exit__(self, *exc):
        self.pds.config.LIN_REG_EXPR_F64 = True


def assert_route(f, pred_mode=0):
    route, info = last_route()
    nb = pc.gate(f.p, len(f.keys), int(f.keys.min()), int(f.keys.max()), np.dtype(f.dtype).itemsize)
    assert route == 1, f"the call did not take the partition route: route {route}, info {info}"
    assert 1 << info[0] == f.B and info[1] == nb and info[3] == pred_mode, (info, f.B, nb)


_DEVICE = {}


def fit(pds, f, space="device"):
    """lin_reg_by_key on the frame; the device-frame result is computed once per frame and shared.  -> (keys, coeffs f64, nulls)"""
    k = (f.p, f.bias, f.dtype)
    if space == "device" and k in _DEVICE:
        return _DEVICE[k]
    put = dev if space == "device" else (lambda a: a)
    with typed(pds, f.dtype):
        r = pds.lin_reg_by_key(*cols_of(f.X, space), target=put(f.y), key=put(f.keys), add_bias=f.bias)
    assert_route(f)
    keys, co, nu = (np_(v) for v in r)
    assert co.dtype == f.dtype
    out = (keys, co.astype(np.float64), nu.astype(bool))
    if space == "device":
        _DEVICE[k] = out
    return out


def check_fit(pds, f, tol):
    keys, co, nu = fit(pds, f)
    t = pc.truth(f)
    assert np.array_equal(keys, np.unique(f.keys))
    assert np.array_equal(nu, f.null), ("null flags", np.flatnonzero(nu != f.null)[:10])
    ok = ~f.null
    d = np.zeros(f.n_groups)
    d[ok] = pc.nrel_rows(co[ok], t[ok])
    worst = {kind: float(d[ok & (f.kind == kind)].max()) for kind in ("light", "heavy", "giant")}
    keys_w = float(d[f.big].max())
    print(f"p={f.p:2d} bias={int(f.bias)} {np.dtype(f.dtype).name}: worst distance light {worst['light']:.2e}  heavy {worst['heavy']:.2e}  "
          f"giant {worst['giant']:.2e}  (the three big keys {keys_w:.2e})")
    assert np.isfinite(co[ok]).all()
    bad = np.flatnonzero(d >= tol)
    assert len(bad) == 0, [(int(g), int(f.uk[g]), str(f.kind[g]), int(f.cnt[g]), float(d[g])) for g in bad[:8]]
    return keys, co, nu


# ------------------------------------------------------------------------------------------------- 1. every width, f64
@pytest.mark.parametrize("p", pc.F64_WIDTHS)
def test_every_width_f64(pds, p):
    """Keys, null flags and every non-null group's coefficients within F64_TOL of the truth, no exceptions; at p in {3, 10, 16} the
    same frame from host memory: same keys and nulls, coefficients within 1e-9 (the records of a bucket arrive in the order of the
    scatter's atomics: two calls agree to rounding, not bit for bit)."""
    f = pc.frame(p, pc.bias_of(p), np.float64)
    keys, co, nu = check_fit(pds, f, pc.F64_TOL)
    if p in pc.HOST_WIDTHS:
        kh, ch, nh = fit(pds, f, "host")
        assert np.array_equal(kh, keys) and np.array_equal(nh, nu)
        ok = ~nu
        assert pc.nrel_rows(ch[ok], co[ok]).max() < 1e-9


# ------------------------------------------------------------------------------------------------- 2. every layout, f32
@pytest.mark.parametrize("p", pc.F32_WIDTHS)
def test_every_layout_f32(pds, p):
    """f32 frames: every instantiation of the accumulate kernel and every f32 record size (1 .. 5 sixteen-byte pieces, padded and
    unpadded), same assertions with F32_TOL against the truth of the f32-rounded data.  This test guards LAYOUT and INDEXING: a
    record piece in the wrong place, a wrong id, a wrong owner.  It cannot see one lost record of the giant group -- that moves beta
    by about 1e-6, a hundredth of F32_TOL; test_every_width_f64 is the one fine enough for that."""
    f = pc.frame(p, pc.bias_of(p), np.float32)
    check_fit(pds, f, pc.F32_TOL)


# ------------------------------------------------------------------------------------------------- 3. per-row predictions
@pytest.mark.parametrize("p,dtype", [(p, np.float64) for p in pc.F64_WIDTHS] + [(p, np.float32) for p, _ in pc.PRED_F32],
                         ids=lambda v: str(v) if isinstance(v, int) else np.dtype(v).name)
def test_pred_every_width(pds, p, dtype):
    """lin_reg_by_key_pred on the same frames: the id-indexed coefficient table (grouped_pred.hip MODE 3) at all three strides -- rows
    padded to 64 bytes (8 f64 / 16 f32 values), to 128 bytes (16 f64 / 32 f32 values), and the unpadded 17 f64 values of p' = 17.  Row flags are the flags of the rows' groups; pred is the route's own coefficients applied to
    the row where it lies, resid = y - pred; rows of null groups are NaN.  Bounds: 1e-12 of ||x|| ||beta|| on f64 frames (the
    coefficients come from a second call: equal to rounding); on f32 frames 4 eps_f32 -- a coefficient may round to the neighbouring
    f32 in the second call (2^-23 of the scale by Cauchy-Schwarz) and pred is rounded once more (2^-24)."""
    bias = pc.bias_of(p)
    f = pc.frame(p, bias, dtype)
    keys, co, nu = fit(pds, f)
    with typed(pds, dtype):
        pr, rs, rn = pds.lin_reg_by_key_pred(*cols_of(f.X), target=dev(f.y), key=dev(f.keys), add_bias=bias)
    assert_route(f, pred_mode=3)
    pr, rs, rn = np_(pr), np_(rs), np_(rn).astype(bool)
    assert pr.dtype == dtype and rs.dtype == dtype
    pr, rs = pr.astype(np.float64), rs.astype(np.float64)
    gi = np.searchsorted(keys, f.keys)
    assert np.array_equal(rn, f.null[gi]) and np.array_equal(nu, f.null)
    assert np.isnan(pr[rn]).all() and np.isnan(rs[rn]).all()
    live = ~rn
    X, y = f.X.astype(np.float64), f.y.astype(np.float64)
    Xb = np.column_stack([X, np.ones(len(X))]) if bias else X
    own = np.einsum("ij,ij->i", Xb[live], co[gi[live]])
    scale = np.linalg.norm(Xb[live], axis=1) * np.linalg.norm(co[gi[live]], axis=1)
    tol = 1e-12 if dtype is np.float64 else 4 * F32_EPS
    e_pred = float(np.max(np.abs(pr[live] - own) / scale))
    e_res = float(np.max(np.abs(rs[live] - (y[live] - own)) / np.maximum(scale, np.abs(y[live]))))
    e_self = float(np.max(np.abs(rs[live] - (y[live] - pr[live])) / np.maximum(scale, np.abs(y[live]))))
    print(f"p={p:2d} bias={int(bias)} {np.dtype(dtype).name}: pred {e_pred:.2e}  resid {e_res:.2e}  resid against y - pred {e_self:.2e}")
    assert e_pred < tol and e_res < tol and e_self < tol


# ------------------------------------------------------------------------------------------------- 4. more buckets than histogram slots
def test_more_buckets_than_slots_exact(pds):
    """16 601 buckets: beyond the 8 192 slots the order check's histogram has, and beyond 64 KiB of LDS for part_hist_kernel's own
    (n_buckets > 16384: the hipFuncSetAttribute branch).  p = 1 without a bias on integer data: Sxx and Sxy are exact integers
    whatever the order of the sums, so beta_g = Sxy / Sxx from np.bincount is the exact reference.  A 1 x 1 solve is at most four
    correctly rounded operations; 8 eps allows twice that."""
    x, y, keys, uk, beta = pc.big_frame()
    r = pds.lin_reg_by_key(dev(x), target=dev(y), key=dev(keys), add_bias=False, max_groups=len(uk))
    route, info = last_route()
    assert route == 1 and info[1] > 16384 and info[2] == 0 and 1 << info[0] == 256, (route, info)
    assert info[1] == pc.gate(1, len(keys), int(keys.min()), int(keys.max()), 8)
    k, co, nu = (np_(v) for v in r)
    assert np.array_equal(k, uk)
    assert not nu.any()
    co = co[:, 0]
    err = np.abs(co - beta)
    eps = np.finfo(np.float64).eps
    rel = err[beta != 0] / np.abs(beta[beta != 0])
    print(f"{len(uk)} groups in {info[1]} buckets: worst |beta - ref| / |ref| = {rel.max() / eps:.2f} eps; "
          f"{np.count_nonzero(err)} of them differ at all")
    assert np.all(err <= 8 * eps * np.abs(beta))
