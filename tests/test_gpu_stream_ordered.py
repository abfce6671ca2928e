"""
Stream-ordered return of the device-resident grouped fit (include/pds_lstsq.h, "Synchronisation"; csrc/grouped_fused.hip,
fixup_marked_kernel).  On a stream the caller handed in, `lin_reg_by` over device columns with up to 16 coefficients queues the
streaming kernel and the marked-group pass behind it and returns; context option "blocking_return" = 1 keeps the route every call
took before -- the host reads the mark word, the count, and drives the Gram / pivoted-QR / scatter kernels itself.  The two routes
must return the SAME BITS, coefficients and flags:

  * 300 groups of 20 .. 40 rows at 3, 8 and 16 f64 features and 8 f32 features, about a tenth of the groups exactly collinear (the
    mark list fires) and a few with fewer rows than features (the null rule fires);
  * three calls on three different frames queued back to back with nothing between them and ONE synchronisation at the end -- a
    pointer table, a mark word or a list slot that a later call rewrites while an earlier kernel still reads it shows here;
  * a frame on which nothing is marked, and one on which every group is marked (the count has no ceiling);
  * a C3-like frame (ragged Poisson group sizes, one group in a hundred collinear) at 8 features;
  * 3 000 marked groups, more batches than the fix-up kernel has blocks; fits with an intercept and with a ridge term.

After every call the hand-over words (marked count, fix-up blocks gone) are back at zero.  Each test asserts through
`Context.last_return_async` that the route it means to exercise is the one that ran.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CASES = [(3, "f64"), (8, "f64"), (16, "f64"), (8, "f32")]


@pytest.fixture(scope="module")
def pds():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import polars_ds_extension_amd as m

    m.config.LIN_REG_EXPR_F64 = True
    yield m
    m.config.LIN_REG_EXPR_F64 = True


@pytest.fixture(scope="module")
def ctx(pds):
    import torch

    c = pds.Context(0)
    c.set_stream(torch.cuda.current_stream())
    yield c
    c.close()


def frame(p, dtype, seed, n_groups=300, collinear=0.1, few=4, sizes=None):
    """Device columns, device offsets and the indices of the collinear / short groups."""
    import torch

    rng = np.random.default_rng(seed)
    if sizes is None:
        sizes = rng.integers(20, 41, size=n_groups)
    n_groups = len(sizes)
    short = rng.choice(n_groups, size=few, replace=False) if few else np.array([], dtype=np.int64)
    sizes = sizes.copy()
    sizes[short] = p - 1
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    N = int(off[-1])
    X = rng.normal(size=(N, p))
    beta = rng.normal(size=(n_groups, p))
    y = np.einsum("ij,ij->i", X, np.repeat(beta, sizes, axis=0)) + 0.1 * rng.normal(size=N)
    coll = np.flatnonzero(rng.random(n_groups) < collinear)
    coll = np.setdiff1d(coll, short)
    for g in coll:  # an exact multiple of another column: the Cholesky breaks down or is gated, the group goes to the marked pass
        X[off[g]: off[g + 1], 1] = 2.0 * X[off[g]: off[g + 1], 0]
    X, y = X.astype(dtype), y.astype(dtype)
    xs = [torch.from_numpy(np.ascontiguousarray(X[:, j])).cuda() for j in range(p)]
    return {"xs": xs, "y": torch.from_numpy(y).cuda(), "off": torch.from_numpy(off).cuda(), "coll": coll, "short": short, "n": n_groups}


def call(pds, ctx, fr, **kw):
    kw.setdefault("add_bias", False)
    return pds.lin_reg_by(*fr["xs"], target=fr["y"], group_offsets=fr["off"], ctx=ctx, **kw)


def blocking(pds, ctx, fr, **kw):
    """The host-driven route, as numpy arrays."""
    ctx.set_option("blocking_return", 1)
    try:
        co, nu = call(pds, ctx, fr, **kw)
        assert not ctx.last_return_async()
    finally:
        ctx.set_option("blocking_return", 0)
    assert ctx.mark_state() == (0, 0)
    return co.cpu().numpy(), nu.cpu().numpy()


def same_bits(got, ref):
    co, nu = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert co.dtype == ref[0].dtype
    assert np.array_equal(nu, ref[1])
    assert np.array_equal(co.view(np.uint64 if co.dtype == np.float64 else np.uint32),
                          ref[0].view(np.uint64 if co.dtype == np.float64 else np.uint32))


@pytest.mark.parametrize("p,kind", CASES)
def test_stream_ordered_equals_blocking(pds, ctx, p, kind):
    pds.config.LIN_REG_EXPR_F64 = kind == "f64"
    try:
        fr = frame(p, np.float64 if kind == "f64" else np.float32, seed=100 + p)
        ref = blocking(pds, ctx, fr)
        assert ref[1][fr["short"]].all() and np.isnan(ref[0][fr["short"]]).all()  # fewer rows than features: null
        assert len(fr["coll"]) >= 15 and ref[1].sum() < fr["n"]
        got = call(pds, ctx, fr)
        assert ctx.last_return_async()
        same_bits(got, ref)
        assert ctx.mark_state() == (0, 0)
    finally:
        pds.config.LIN_REG_EXPR_F64 = True


@pytest.mark.parametrize("p,kind", CASES)
def test_three_calls_queued_back_to_back(pds, ctx, p, kind):
    import torch

    pds.config.LIN_REG_EXPR_F64 = kind == "f64"
    try:
        dtype = np.float64 if kind == "f64" else np.float32
        frames = [frame(p, dtype, seed=200 + 10 * p + k, n_groups=n) for k, n in enumerate((300, 270, 320))]
        refs = [blocking(pds, ctx, fr) for fr in frames]
        torch.cuda.synchronize()
        outs = []
        for fr in frames:  # nothing between the calls: device inputs, device offsets, no read-back
            outs.append(call(pds, ctx, fr))
            assert ctx.last_return_async()
        torch.cuda.synchronize()
        for got, ref in zip(outs, refs):
            same_bits(got, ref)
        assert ctx.mark_state() == (0, 0)
    finally:
        pds.config.LIN_REG_EXPR_F64 = True


def test_nothing_marked_and_everything_marked(pds, ctx):
    none = frame(8, np.float64, seed=31, collinear=0.0, few=0)
    ref = blocking(pds, ctx, none)
    assert not ref[1].any()
    got = call(pds, ctx, none)
    assert ctx.last_return_async()
    same_bits(got, ref)
    assert ctx.mark_state() == (0, 0)
    every = frame(8, np.float64, seed=32, collinear=2.0, few=0)
    assert len(every["coll"]) == every["n"]
    ref = blocking(pds, ctx, every)
    got = call(pds, ctx, every)
    assert ctx.last_return_async()
    same_bits(got, ref)
    assert ctx.mark_state() == (0, 0)
    # and the first frame once more behind it: the count the second call ran up is gone
    same_bits(call(pds, ctx, none), blocking(pds, ctx, none))


@pytest.mark.parametrize("p", [8, 16])
def test_more_marked_batches_than_fix_up_blocks(pds, ctx, p):
    """The fix-up kernel's grid is one block per compute unit (256 on the MI355X) and a block takes 64 / LPS marked groups per
    pass: 3 000 marked groups are 375 batches at 8 features and 750 at 16, so blocks go round their loop a second and third time."""
    fr = frame(p, np.float64, seed=40 + p, n_groups=3000, collinear=2.0, few=0)
    assert len(fr["coll"]) == 3000 and 3000 // (64 // p) > 256
    ref = blocking(pds, ctx, fr)
    got = call(pds, ctx, fr)
    assert ctx.last_return_async()
    same_bits(got, ref)
    assert ctx.mark_state() == (0, 0)


@pytest.mark.parametrize("p,kw", [(3, {"add_bias": True}), (8, {"add_bias": True}), (15, {"add_bias": True}), (8, {"l2_reg": 1e-10}),
                                  (7, {"add_bias": True, "l2_reg": 1e-10})])
def test_intercept_and_ridge(pds, ctx, p, kw):
    """Coefficient count != feature count: the fix-up's solver width follows p + 1 (3 + 1 -> 4 lanes, 8 + 1 and 15 + 1 -> 16, 7 + 1 -> 8)
    while its Gram record follows p, and a ridge term goes onto the feature diagonals only.  (16 features + intercept keep the
    host-driven pass: test_routes_that_keep_the_blocking_return.)"""
    fr = frame(p, np.float64, seed=60 + p)
    ref = blocking(pds, ctx, fr, **kw)
    got = call(pds, ctx, fr, **kw)
    assert ctx.last_return_async()
    same_bits(got, ref)
    assert ctx.mark_state() == (0, 0)


def test_c3_like_frame(pds, ctx):
    rng = np.random.default_rng(33)
    sizes = np.clip(rng.poisson(100, size=3000), 16, 256)
    fr = frame(8, np.float64, seed=34, collinear=0.01, few=0, sizes=sizes)
    assert len(fr["coll"]) >= 10
    ref = blocking(pds, ctx, fr)
    got = call(pds, ctx, fr)
    assert ctx.last_return_async()
    same_bits(got, ref)
    assert ctx.mark_state() == (0, 0)


def test_routes_that_keep_the_blocking_return(pds, ctx):
    """solver = "svd" (host SVD threads), 16 features with an intercept (17 coefficients: the LDS solver), host frames and a context
    on its own stream all synchronise before they return, as before; "choleskey" marks nothing and stays on the stream."""
    fr = frame(8, np.float64, seed=35)
    call(pds, ctx, fr, solver="svd")
    assert not ctx.last_return_async()
    co_c, nu_c = call(pds, ctx, fr, solver="choleskey")
    assert ctx.last_return_async()
    ctx.set_option("blocking_return", 1)
    try:
        ref = call(pds, ctx, fr, solver="choleskey")
    finally:
        ctx.set_option("blocking_return", 0)
    same_bits((co_c, nu_c), (ref[0].cpu().numpy(), ref[1].cpu().numpy()))
    f16 = frame(16, np.float64, seed=36)
    pds.lin_reg_by(*f16["xs"], target=f16["y"], group_offsets=f16["off"], add_bias=True, ctx=ctx)
    assert not ctx.last_return_async()
    host = pds.lin_reg_by(*[x.cpu().numpy() for x in fr["xs"]], target=fr["y"].cpu().numpy(), group_offsets=fr["off"].cpu().numpy(), ctx=ctx)
    assert not ctx.last_return_async()
    same_bits(call(pds, ctx, fr), (np.asarray(host[0]), np.asarray(host[1])))
    own = pds.Context(0, follow_torch=False)  # never given a stream, and told not to take torch's: its private one
    try:
        import torch

        torch.cuda.synchronize()  # (the inputs were produced on torch's stream)
        got = call(pds, own, fr)
        assert not own.last_return_async()
        same_bits(call(pds, ctx, fr), (got[0].cpu().numpy(), got[1].cpu().numpy()))
    finally:
        own.close()


def test_option_range(pds, ctx):
    from polars_ds_extension_amd import _lib

    with pytest.raises(_lib.PdsError):
        ctx.set_option("blocking_return", 2)
    assert ctx.get_option("blocking_return") == 0
