"""
Host frames against device frames, bit for bit, for every grouped entry point.

A host frame (NumPy columns, NumPy outputs) takes the same kernels as a device frame (CUDA tensors); what differs is the host side
of the pipeline: the columns go up into a workspace, every output is written to a workspace slice and copied back.  A slice whose
size, position or copy count is wrong shows as different bits (or as a workspace spill), so every returned array is compared on
its raw bytes -- NaN patterns of null groups included -- and pds_ctx_workspace_spills must stay 0.

The frame: 1 531 rows (a prime: no column is a multiple of 256 bytes), 3 features with and without a bias, 37 distinct keys with
uneven group sizes, one group with fewer rows than coefficients (null flags and NaNs travel through the copies).  The offsets forms
get one EMPTY group on top (38 groups: a key column cannot name a group without rows).  The by-key forms run on ascending keys and
on a fixed permutation of the rows (sort + gather + scatter back), with max_groups = 37 (the copy count equals the capacity) and
64 (it does not).  f64 everywhere, one f32 case per family.
"""
import contextlib
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_ROWS, N_KEYS, P = 1531, 37, 3
DTYPES = [(np.float64, False), (np.float64, True), (np.float32, True)]  # (precision, add_bias)
ORDERS = ["ascending", "permuted"]


@pytest.fixture(scope="module")
def pds():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import polars_ds_extension_amd as m

    return m


@pytest.fixture(scope="module")
def ctx(pds):
    """one context for the module: "keyed_sort" makes lin_reg_by_key's route for unordered keys reproducible to the bit"""
    from polars_ds_extension_amd import lstsq

    c = lstsq.Context(0)
    c.set_option("keyed_sort", 1)
    yield c
    c.close()


class Frame:
    def __init__(self):
        rng = np.random.default_rng(1531)
        cuts = np.sort(rng.choice(np.arange(1, N_ROWS - 2), size=N_KEYS - 2, replace=False))
        sizes = np.diff(np.concatenate([[0], cuts, [N_ROWS - 2]]))
        sizes = np.concatenate([sizes[:11], [2], sizes[11:]])  # group 11: 2 rows < 3 coefficients
        assert len(sizes) == N_KEYS and sizes.sum() == N_ROWS and sizes.min() >= 1 and len(set(sizes.tolist())) > 10
        self.sizes = sizes
        self.labels = (np.arange(N_KEYS, dtype=np.int64) * 5 - 40)
        self.key = np.repeat(self.labels, sizes)
        off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        self.off = np.concatenate([off[:20], [off[20]], off[20:]])  # + an empty group in front of group 20
        assert len(self.off) == N_KEYS + 2
        self.X = rng.normal(size=(N_ROWS, P))
        beta = np.array([0.7, -1.1, 0.4])
        self.y = self.X @ beta + 0.3 + 0.2 * rng.normal(size=N_ROWS)
        self.yb = (self.X @ beta + 0.5 * rng.logistic(size=N_ROWS) > 0).astype(np.float64)
        self.w = rng.uniform(0.5, 2.0, size=N_ROWS)
        self.perm = np.random.default_rng(7).permutation(N_ROWS)

    def rows(self, order):
        return self.perm if order == "permuted" else np.arange(N_ROWS)

    def small(self, pp, offsets_form=False):
        """groups with fewer rows than coefficients: null (the 2-row group, whatever the cuts left as small, the empty group)"""
        return (np.diff(self.off) if offsets_form else self.sizes) < pp


FRAME = Frame()


def dev(a):
    import torch

    return torch.from_numpy(np.array(a, order="C")).cuda()


def np_(v):
    return v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)


@contextlib.contextmanager
def precision(pds, dt):
    pds.config.LIN_REG_EXPR_F64 = dt == np.float64
    try:
        yield
    finally:
        pds.config.LIN_REG_EXPR_F64 = True


def arrays(r):
    """the arrays of a result (tuple or dict), named"""
    if isinstance(r, dict):
        return {k: np_(v) for k, v in r.items() if k != "features"}
    return {str(i): np_(v) for i, v in enumerate(r)}


def spills(ctx):
    return int(ctx._lib.pds_ctx_workspace_spills(ctx._h))


def same_bits(pds, ctx, dt, call, rows=None):
    """call(put, cols): `put` places one array, `cols(M)` the columns of a matrix, in the space under test"""
    rows = FRAME.rows("ascending") if rows is None else rows
    got = {}
    before = spills(ctx)
    with precision(pds, dt):
        for space in ("host", "device"):
            put = (lambda a: dev(a[rows])) if space == "device" else (lambda a: np.ascontiguousarray(a[rows]))
            cast = lambda a: put(np.asarray(a, dtype=dt))  # noqa: E731
            got[space] = arrays(call(cast, lambda M: [cast(M[:, j]) for j in range(M.shape[1])]))
    h, d = got["host"], got["device"]
    assert h.keys() == d.keys() and len(h) > 0
    for k in h:
        assert h[k].dtype == d[k].dtype and h[k].shape == d[k].shape, k
        assert np.array_equal(np.ascontiguousarray(h[k]).reshape(-1).view(np.uint8), np.ascontiguousarray(d[k]).reshape(-1).view(np.uint8)), k
    assert spills(ctx) == before == 0
    return h


# ------------------------------------------------------------------------------------------------- lin_reg_by / _pred
@pytest.mark.parametrize("dt,bias", DTYPES)
@pytest.mark.parametrize("variant", ["plain", "weights", "l1"])
def test_lin_reg_by(pds, ctx, dt, bias, variant):
    f = FRAME
    kw = {"weights": "w"} if variant == "weights" else ({"l1_reg": 0.01} if variant == "l1" else {})

    def call(put, cols):
        k = dict(kw)
        if "weights" in k:
            k["weights"] = put(f.w)
        return pds.lin_reg_by(*cols(f.X), target=put(f.y), group_offsets=f.off, add_bias=bias, ctx=ctx, **k)

    r = same_bits(pds, ctx, dt, call)
    nu = r["1"].astype(bool)
    assert r["0"].shape == (N_KEYS + 1, P + bias) and np.isfinite(r["0"][~nu]).all() and not nu.all()
    if variant == "plain":
        assert nu[11] and nu[20] and np.array_equal(nu, f.small(P + bias, True)) and np.isnan(r["0"][nu]).all()  # (2 rows; the empty group)


@pytest.mark.parametrize("dt,bias", DTYPES)
@pytest.mark.parametrize("weighted", [False, True])
def test_lin_reg_by_pred(pds, ctx, dt, bias, weighted):
    f = FRAME
    r = same_bits(pds, ctx, dt, lambda put, cols: pds.lin_reg_by_pred(*cols(f.X), target=put(f.y), group_offsets=f.off, add_bias=bias,
                                                                      weights=put(f.w) if weighted else None, ctx=ctx))
    assert r["0"].shape == (N_ROWS,) and r["3"].shape == (N_KEYS + 1, P + bias) and np.isnan(r["0"][r["2"].astype(bool)]).all()
    if not weighted:
        assert r["2"].sum() == f.sizes[f.small(P + bias)].sum() >= 2  # the rows of the small groups


# ------------------------------------------------------------------------------------------------- lin_reg_by_key / _pred
@pytest.mark.parametrize("dt,bias", DTYPES)
@pytest.mark.parametrize("max_groups", [N_KEYS, 64])
@pytest.mark.parametrize("order", ORDERS)
def test_lin_reg_by_key(pds, ctx, dt, bias, order, max_groups):
    f = FRAME
    rows = f.rows(order)
    r = same_bits(pds, ctx, dt, lambda put, cols: pds.lin_reg_by_key(*cols(f.X), target=put(f.y), key=f.key[rows], add_bias=bias,
                                                                     max_groups=max_groups, ctx=ctx), rows)
    assert np.array_equal(r["0"], f.labels) and r["1"].shape == (N_KEYS, P + bias) and np.array_equal(r["2"].astype(bool), f.small(P + bias))


@pytest.mark.parametrize("dt,bias", DTYPES)
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("order", ORDERS)
def test_lin_reg_by_key_pred(pds, ctx, dt, bias, order, weighted):
    f = FRAME
    rows = f.rows(order)
    r = same_bits(pds, ctx, dt, lambda put, cols: pds.lin_reg_by_key_pred(*cols(f.X), target=put(f.y), key=f.key[rows], add_bias=bias,
                                                                          weights=put(f.w) if weighted else None, ctx=ctx), rows)
    assert r["0"].shape == (N_ROWS,) and np.isnan(r["0"][r["2"].astype(bool)]).all()
    if not weighted:
        assert np.array_equal(r["2"].astype(bool), np.repeat(f.small(P + bias), f.sizes)[rows])  # null rows where the rows ARE


# ------------------------------------------------------------------------------------------------- reports
REPORTS = [("se", False), ("hc2", False), ("se", True)]  # (std_err, weighted)


@pytest.mark.parametrize("dt,bias", DTYPES)
@pytest.mark.parametrize("std_err,weighted", REPORTS)
def test_lin_reg_report_by(pds, ctx, dt, bias, std_err, weighted):
    f = FRAME
    r = same_bits(pds, ctx, dt, lambda put, cols: pds.lin_reg_report_by(*cols(f.X), target=put(f.y), group_offsets=f.off, add_bias=bias,
                                                                        std_err=std_err, weights=put(f.w) if weighted else None, ctx=ctx))
    assert len(r) == 9 and r["is_null"][11] and r["is_null"][20] and np.isnan(r["beta"][11]).all()


@pytest.mark.parametrize("dt,bias", DTYPES)
@pytest.mark.parametrize("std_err,weighted", REPORTS)
@pytest.mark.parametrize("max_groups", [N_KEYS, 64])
@pytest.mark.parametrize("order", ORDERS)
def test_lin_reg_report_by_key(pds, ctx, dt, bias, order, max_groups, std_err, weighted):
    f = FRAME
    rows = f.rows(order)
    r = same_bits(pds, ctx, dt, lambda put, cols: pds.lin_reg_report_by_key(*cols(f.X), target=put(f.y), key=f.key[rows], add_bias=bias,
                                                                            std_err=std_err, weights=put(f.w) if weighted else None,
                                                                            max_groups=max_groups, ctx=ctx), rows)
    assert len(r) == 10 and np.array_equal(r["keys"], f.labels) and r["beta"].shape == (N_KEYS, P + bias) and np.array_equal(r["is_null"].astype(bool), f.small(P + bias))


# ------------------------------------------------------------------------------------------------- rolling / recursive
@pytest.mark.parametrize("dt,bias", DTYPES)
@pytest.mark.parametrize("kind", ["rolling", "recursive"])
def test_windowed_by(pds, ctx, dt, bias, kind):
    f = FRAME
    fn = getattr(pds, f"{kind}_lin_reg_by")
    kw = {"window_size": 9} if kind == "rolling" else {"start_with": 6}
    r = same_bits(pds, ctx, dt, lambda put, cols: fn(*cols(f.X), target=put(f.y), group_offsets=f.off, add_bias=bias, ctx=ctx, **kw))
    assert r["0"].shape == (N_ROWS, P + bias) and 0 < r["2"].sum() < N_ROWS


@pytest.mark.parametrize("dt,bias", DTYPES)
@pytest.mark.parametrize("kind", ["rolling", "recursive"])
@pytest.mark.parametrize("order", ORDERS)
def test_windowed_by_key(pds, ctx, dt, bias, order, kind):
    f = FRAME
    rows = f.rows(order)
    fn = getattr(pds, f"{kind}_lin_reg_by_key")
    kw = {"window_size": 9} if kind == "rolling" else {"start_with": 6}
    r = same_bits(pds, ctx, dt, lambda put, cols: fn(*cols(f.X), target=put(f.y), key=f.key[rows], add_bias=bias, ctx=ctx, **kw), rows)
    assert r["0"].shape == (N_ROWS, P + bias) and 0 < r["2"].sum() < N_ROWS


# ------------------------------------------------------------------------------------------------- GLM (logistic, per-row outputs)
@pytest.mark.parametrize("dt,bias", DTYPES)
@pytest.mark.parametrize("return_pred", [True, False])
def test_glm_by(pds, ctx, dt, bias, return_pred):
    f = FRAME
    r = same_bits(pds, ctx, dt, lambda put, cols: pds.glm_by(*cols(f.X), target=put(f.yb), group_offsets=f.off, family="binomial", add_bias=bias,
                                                             return_pred=return_pred, ctx=ctx))
    assert len(r) == (5 if return_pred else 3) and r["2"][11] and r["2"][20] and not r["2"].all()


@pytest.mark.parametrize("dt,bias", DTYPES)
@pytest.mark.parametrize("max_groups", [N_KEYS, 64])
@pytest.mark.parametrize("order", ORDERS)
def test_glm_by_key(pds, ctx, dt, bias, order, max_groups):
    f = FRAME
    rows = f.rows(order)
    r = same_bits(pds, ctx, dt, lambda put, cols: pds.glm_by_key(*cols(f.X), target=put(f.yb), key=f.key[rows], family="binomial", add_bias=bias,
                                                                 return_pred=True, max_groups=max_groups, ctx=ctx), rows)
    assert len(r) == 6 and np.array_equal(r["0"], f.labels) and r["3"][11] and not r["3"].all()
    assert r["5"][f.key[rows] == f.labels[11]].all()


# ------------------------------------------------------------------------------------------------- lin_reg_w_rcond
@pytest.mark.parametrize("dt,bias", DTYPES)
def test_rcond_by(pds, ctx, dt, bias):
    f = FRAME
    r = same_bits(pds, ctx, dt, lambda put, cols: pds.lin_reg_w_rcond_by(*cols(f.X), target=put(f.y), group_offsets=f.off, add_bias=bias,
                                                                         rcond=1e-6, ctx=ctx))
    assert r["2"][11] and r["2"][20] and np.array_equal(r["2"].astype(bool), f.small(P + bias, True)) and np.isnan(r["1"][11]).all()


@pytest.mark.parametrize("dt,bias", DTYPES)
@pytest.mark.parametrize("max_groups", [N_KEYS, 64])
@pytest.mark.parametrize("order", ORDERS)
def test_rcond_by_key(pds, ctx, dt, bias, order, max_groups):
    f = FRAME
    rows = f.rows(order)
    r = same_bits(pds, ctx, dt, lambda put, cols: pds.lin_reg_w_rcond_by_key(*cols(f.X), target=put(f.y), key=f.key[rows], add_bias=bias,
                                                                             rcond=1e-6, max_groups=max_groups, ctx=ctx), rows)
    assert np.array_equal(r["0"], f.labels) and np.array_equal(r["3"].astype(bool), f.small(P + bias)) and r["3"][11]


# ------------------------------------------------------------------------------------------------- mixed model
@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("order", ORDERS)
def test_mixed_reml_by_key(pds, ctx, dt, order):
    f = FRAME
    rows = f.rows(order)
    r = same_bits(pds, ctx, dt, lambda put, cols: pds.mixed_reml(*cols(f.X), target=put(f.y), key=f.key[rows], ctx=ctx), rows)
    assert int(r["n_groups"]) == N_KEYS and np.isfinite(r["coeffs"]).all()


# ------------------------------------------------------------------------------------------------- the partition route, host frame
def test_partition_route_host_frame(pds):
    """Dense keys in shuffled rows, >= 2^17 rows, 2 features, "keyed_sort" off: lin_reg_by_key's partition route (the shape conditions of
    test_gpu_parity.py::test_by_key_pred_partition_route).  Its record order follows cursor atomics, so two runs agree to rounding,
    not to the bit: keys and null flags are equal, coefficients and predictions within the 1e-9 test_gpu_parity.py holds that route
    to against the sorting route."""
    from polars_ds_extension_amd import lstsq

    rng = np.random.default_rng(217)
    G, p = 2000, 2
    sizes = rng.integers(40, 100, size=G)
    sizes[::97] = 1  # fewer rows than coefficients: null
    key = rng.permutation(np.repeat(np.arange(G, dtype=np.int64) + 100, sizes))
    N = len(key)
    assert N >= 1 << 17
    X = rng.normal(size=(N, p))
    y = X @ np.array([0.5, -0.25]) + 1e-3 * key + 0.1 * rng.normal(size=N)
    c = lstsq.Context(0)
    try:
        c.set_option("keyed_sort", 0)
        hk, hc, hn = pds.lin_reg_by_key(X[:, 0].copy(), X[:, 1].copy(), target=y, key=key, add_bias=True, ctx=c)
        hp, hr, hrn = pds.lin_reg_by_key_pred(X[:, 0].copy(), X[:, 1].copy(), target=y, key=key, add_bias=True, ctx=c)
        dk, dc, dn = (np_(v) for v in pds.lin_reg_by_key(dev(X[:, 0]), dev(X[:, 1]), target=dev(y), key=dev(key), add_bias=True, ctx=c))
        dp, dr, drn = (np_(v) for v in pds.lin_reg_by_key_pred(dev(X[:, 0]), dev(X[:, 1]), target=dev(y), key=dev(key), add_bias=True, ctx=c))
        assert spills(c) == 0
    finally:
        c.close()
    assert isinstance(hc, np.ndarray) and isinstance(hp, np.ndarray)
    assert np.array_equal(hk, np.arange(G) + 100) and np.array_equal(hk, dk)
    assert np.array_equal(hn, dn) and hn.sum() == len(sizes[::97])
    assert np.array_equal(hrn, drn) and hrn.sum() == len(sizes[::97])
    ok, rok = ~hn.astype(bool), ~hrn.astype(bool)
    assert np.isnan(hc[~ok]).all() and np.isnan(dc[~ok]).all() and np.isnan(hp[~rok]).all() and np.isnan(dp[~rok]).all()
    print(f"partition route host vs device: coeffs {np.max(np.abs(hc[ok] - dc[ok])):.3e} pred {np.max(np.abs(hp[rok] - dp[rok])):.3e}")
    assert np.max(np.abs(hc[ok] - dc[ok])) < 1e-9
    assert np.max(np.abs(hp[rok] - dp[rok])) < 1e-9 and np.max(np.abs(hr[rok] - dr[rok])) < 1e-9


# ------------------------------------------------------------------------------------------------- the retry contract
@pytest.mark.parametrize("space", ["host", "device"])
def test_max_groups_too_small_reports_the_count(pds, ctx, space):
    """max_groups = 5 on the 37-key frame: PDS_ERR_INVALID "more distinct keys than max_groups", and *n_groups already holds 37 --
    what lstsq._by_key_retry grows its outputs from."""
    from polars_ds_extension_amd import _lib, lstsq

    f = FRAME
    put = dev if space == "device" else np.ascontiguousarray
    cols = lstsq._Cols(put(f.y), [put(f.X[:, j]) for j in range(P)])
    key = put(f.key)
    cap, pp = 5, P + 1
    outs = [put(np.zeros(cap, np.int64)), put(np.zeros((cap, pp))), put(np.zeros((cap, pp))), put(np.zeros(cap, np.uint8))]
    addr = lambda a: C.c_void_p(int(a.data_ptr()) if hasattr(a, "data_ptr") else a.ctypes.data)  # noqa: E731
    ng = C.c_int64(0)
    rcode = ctx._lib.pds_lr_rcond_by_key_f64(ctx._h, cols.cols, addr(key), P, C.c_int64(N_ROWS), cols.space, 1, C.c_double(0.0), C.c_double(1e-6),
                                             C.c_int64(cap), addr(outs[0]), addr(outs[1]), addr(outs[2]), addr(outs[3]), C.byref(ng))
    assert rcode == -1 and ng.value == N_KEYS  # PDS_ERR_INVALID
    assert "more distinct keys than max_groups" in ctx._lib.pds_last_error().decode()
    with pytest.raises(_lib.PdsError, match="more distinct keys than max_groups"):
        pds.lin_reg_w_rcond_by_key(*[put(f.X[:, j]) for j in range(P)], target=put(f.y), key=key, add_bias=True, max_groups=cap, ctx=ctx)
