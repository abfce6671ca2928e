"""The streaming kernels of the one-model path and grouped_pred_kernel with MORE THAN ONE unit of work per wave.

Their grids are fixed multiples of the CU count, so at the row counts of the other parity tests a wave gets zero or one unit and the
loop that prefetches unit t + 1 while unit t is consumed -- and carries accumulators, per-lane side sums and the group cursor from one
unit to the next -- never turns.  tests/steady_cases.py takes the row counts from the launchers' own work split (2 .. 3 units per wave
plus a ragged tail, for the CU count of the device at hand); tests/test_steady_shapes_cpu.py pins that arithmetic without a GPU.

Every tolerance is one the suite already holds at equal or larger row counts (named at each test); the Gram tests need none: on
integer frames every partial sum is an integer below 2^24, exact in f32 and f64 under any summation order."""
import contextlib
import functools
import os
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))
import steady_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu

F64_TOL = 1e-10
F32_TOL = 1e-4
F64, F32 = sc.F64, sc.F32


@pytest.fixture(scope="module")
def pds():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import polars_ds_extension_amd as m

    m.config.LIN_REG_EXPR_F64 = True
    return m


@pytest.fixture(scope="module")
def cus(pds):
    return pds.default_context().num_cus


@contextlib.contextmanager
def precision(pds, dtype):
    pds.config.LIN_REG_EXPR_F64 = np.dtype(dtype) == np.float64
    try:
        yield
    finally:
        pds.config.LIN_REG_EXPR_F64 = True


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def cols_of(X):
    return [dev(X[:, j]) for j in range(X.shape[1])]


def nrel(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def frel(a, b, floor=1e-12):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), floor)))


def hold_f32(name, gpu, o32, truth, d=None, slack=1.25):
    """The f32 contract (tests/test_f32_contract.py, test_gpu_parity.hold_f32): within 1e-4 of the f64 truth, or -- where the
    reference's own all-f32 arithmetic is further than that from the truth -- no further than the reference's f32 path is."""
    d = d or nrel
    dg, do = d(gpu, truth), d(o32, truth)
    print(f"{name}: gpu-truth {dg:.2e}  orc32-truth {do:.2e}")
    assert dg <= F32_TOL or (do > F32_TOL and dg <= do * slack), f"{name}: gpu-truth {dg:.2e}, orc32-truth {do:.2e}"


def se_key(se):
    return "std_err" if se == "se" else f"{se}_se"


# ------------------------------------------------------------------------------------------ 2. exact Gram on integer frames
@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("p", sc.SMALL_P + sc.MID_P)
def test_gram_is_exact_on_integer_frames(pds, cus, p, dtype):
    """moments_small_kernel (every packing and the 16-feature form, with and without the weight column) and moments_mid_kernel
    (NBLK = 2 and 4), both precisions: features and target in [-3, 3], weights in {0, 1} -- the Gram of [X | 1 | y] equals the integer
    Gram, bit for bit, at 2 .. 3 units per wave plus a ragged tail, and at the sizes where every wave has exactly one unit, where one
    wave has two, and one row beyond."""
    kind = "small" if p <= 16 else "mid"
    sizes = [sc.rows(kind, dtype, p, cus)]
    if p in sc.BOUNDARY_P:
        sizes += [b[0] for b in sc.boundary_rows(kind, dtype, p, cus)]
    nmax = max(sizes)
    assert 9 * nmax < 2 ** 24, "a partial sum could leave f32's integers: shrink `units`"
    X, y, w = sc.integer_frame(1000 * p + np.dtype(dtype).itemsize, nmax, p, dtype)
    cols, ty, tw = cols_of(X), dev(y), dev(w)
    Z = sc.integer_design(X, y)
    with precision(pds, dtype):
        for n in sizes:
            u = sc.units_per_wave(kind, dtype, p, n, cus)
            cn, yn, wn = [c[:n] for c in cols], ty[:n], tw[:n]
            for weights in (None, wn):
                ref = sc.gram_of_design(Z[:n], None if weights is None else w[:n])
                M = pds.gram_moments(*cn, target=yn, weights=weights)
                assert M.dtype == np.dtype(dtype) and M.shape == (p + 2, p + 2)
                bad = np.argwhere(M.astype(np.float64) != ref.astype(np.float64))
                assert bad.size == 0, (n, weights is not None, int(u.min()), int(u.max()), bad[:5].tolist(),
                                       [(float(M[i, j]), int(ref[i, j])) for i, j in bad[:5]])
                assert np.array_equal(M, pds.gram_moments(*cn, target=yn, weights=weights)), (n, weights is not None)


# ------------------------------------------------------------------------------------------ 3. derived-weight passes, <= 16 features
@functools.lru_cache(maxsize=1)
def _report_case(p, bias, dtype, n):
    X, y = sc.report_frame(50 + p, n, p, bias)
    X, y = X.astype(dtype), y.astype(dtype)
    return X, y, cols_of(X), dev(y)


def check_report_f64(r, ro, se, n, pp, orc):
    """The bars of test_gpu_parity.test_lin_reg_report / test_baseline_sizes.test_c2_prefix_against_oracle: beta 1e-10 normwise, standard
    errors 1e-10 elementwise, t / p / CI by the bounds those propagate, r2 at 1e-12."""
    from scipy import stats

    beta_o, se_o, t_o = np.asarray(ro["beta"]), np.asarray(ro["std_err"]), np.asarray(ro["t"])
    e_b, e_s = nrel(r["beta"], beta_o), frel(r[se_key(se)], se_o)
    print(f"beta {e_b:.2e}  {se} {e_s:.2e}  r2 {abs(r['r2'][0] - ro['r2']):.2e}")
    assert e_b < F64_TOL and e_s < F64_TOL
    dt_bound = F64_TOL * (np.linalg.norm(beta_o) / se_o + np.abs(t_o))
    assert np.all(np.abs(np.asarray(r["t"]) - t_o) <= dt_bound)
    dof = float(n - pp)
    dp_bound = 2.0 * stats.t.pdf(np.abs(t_o), dof) * dt_bound + 1e-14 * np.asarray(ro["p"])
    assert np.all(np.abs(np.asarray(r["p>|t|"]) - np.asarray(ro["p"])) <= dp_bound)
    t_crit = float(orc.student_t_ppf(0.975, dof))
    ci_bound = F64_TOL * (np.linalg.norm(beta_o) + t_crit * se_o)
    assert np.all(np.abs(np.asarray(r["0.025"]) - np.asarray(ro["ci_lo"])) <= ci_bound)
    assert np.all(np.abs(np.asarray(r["0.975"]) - np.asarray(ro["ci_hi"])) <= ci_bound)
    assert abs(r["r2"][0] - ro["r2"]) < 1e-12 and abs(r["adj_r2"][0] - ro["adj_r2"]) < 1e-12


@pytest.mark.parametrize("p,bias,se", sc.REPORT_CASES)
def test_report_every_width(pds, orc, cus, p, bias, se):
    """lin_reg_report at every width of moments_small_kernel: SE (pass2_kernel's double-buffered register sets, every PC), HC0 / HC1
    (WM = 2: residual weights and the side sums of y formed per tile, every packing) and HC2 / HC3 (WM = 4: leverages on the matrix
    cores between the store of tile t and the load of tile t + 1); var(y) is the library's own (sums carried per lane across tiles)."""
    n = sc.rows("small", F64, p, cus)
    X, y, cols, ty = _report_case(p, bias, F64, n)
    r = pds.lin_reg_report(*cols, target=ty, add_bias=bias, std_err=se)
    ro = orc.lin_reg_report(np.c_[X, np.ones(n)] if bias else X, y, std_err=se)
    check_report_f64(r, ro, se, n, p + int(bias), orc)


@pytest.mark.parametrize("se", ["hc1", "hc3"])
@pytest.mark.parametrize("p", sc.REPORT_F32_P)
def test_report_f32(pds, orc, cus, p, se):
    n = sc.rows("small", F32, p, cus)
    X32, y32, cols, ty = _report_case(p, True, F32, n)
    with precision(pds, F32):
        r = pds.lin_reg_report(*cols, target=ty, add_bias=True, std_err=se)
    assert r["beta"].dtype == np.float32
    ro32 = orc.lin_reg_report(np.c_[X32, np.ones(n, np.float32)], y32, std_err=se)
    ro = orc.lin_reg_report(np.c_[X32.astype(np.float64), np.ones(n)], y32.astype(np.float64), std_err=se)
    hold_f32(f"report f32 p={p} {se}: std err", r[se_key(se)], ro32["std_err"], ro["std_err"], frel)
    hold_f32(f"report f32 p={p} {se}: beta", r["beta"], ro32["beta"], ro["beta"])


@pytest.mark.parametrize("p,dtype", sc.WLS_CASES)
def test_wls_report_and_pred(pds, orc, cus, p, dtype):
    """The weight column from memory (WM = 1) in the Gram build and in pass2_kernel<WEIGHTED>; pred / resid written by the double-buffered
    loop: pred is the returned coefficients applied to the row, resid is y - pred to the bit."""
    n = sc.rows("small", dtype, p, cus)
    X, y, cols, ty = _report_case(p, True, dtype, n)
    w = (np.random.default_rng(70 + p).random(n) + 0.1).astype(dtype)
    tw = dev(w)
    X64, y64, w64 = X.astype(np.float64), y.astype(np.float64), w.astype(np.float64)
    Xb = np.c_[X64, np.ones(n)]
    with precision(pds, dtype):
        r = pds.lin_reg_report(*cols, target=ty, add_bias=True, weights=tw, y_var=float(np.var(y64, ddof=1)))
        b = pds.lin_reg(*cols, target=ty, add_bias=True, weights=tw)
        pred, resid = pds.lin_reg(*cols, target=ty, add_bias=True, weights=tw, return_pred=True)
    ro = orc.wls_report(Xb, y64, w64)
    pred, resid = pred.cpu().numpy(), resid.cpu().numpy()
    assert pred.dtype == np.dtype(dtype) and b.dtype == np.dtype(dtype)
    own = Xb @ b.astype(np.float64)
    scale = np.linalg.norm(Xb, axis=1) * np.linalg.norm(b)
    if dtype == F64:  # test_wls_report's bars; pred by test_grouped_pred's bound for the same statement
        assert nrel(r["beta"], ro["beta"]) < F64_TOL and frel(r["std_err"], ro["std_err"]) < F64_TOL
        assert frel(r["p>|t|"], ro["p"]) < 1e-8 and abs(r["r2"][0] - ro["r2"]) < 1e-12
        np.testing.assert_allclose(pred, own, rtol=1e-12, atol=1e-12 * np.max(scale))
    else:
        ro32 = orc.wls_report(np.c_[X, np.ones(n, np.float32)], y, w)
        hold_f32(f"wls f32 p={p}: beta", r["beta"], ro32["beta"], ro["beta"])
        hold_f32(f"wls f32 p={p}: std err", r["std_err"], ro32["std_err"], ro["std_err"], frel)
        # an f32 dot product of p' terms: |fl(x . b) - x . b| <= gamma_p' |x|' |b| <= (p' + 1) 2^-24 |x| |b| (Higham, Accuracy and
        # Stability of Numerical Algorithms, (3.5)); the f64 product it is compared with errs by 1e-16 of the same
        assert np.all(np.abs(pred.astype(np.float64) - own) <= (p + 2) * 2.0 ** -24 * scale)
    assert np.array_equal(resid, y - pred)  # one subtraction in the frame's precision: nothing to round differently


@pytest.mark.parametrize("p,family,bias", sc.GLM_CASES)
def test_glm_every_width(pds, orc, cus, p, family, bias):
    """GLM.fit (one model): every IRLS step is one moments_small_kernel<WM = 3> pass -- weights and working response from the previous
    coefficients while the tile is in registers.  Bars of test_linear_models.test_glm_matches_the_oracle."""
    import torch

    from polars_ds_extension_amd.linear_models import GLM

    n = sc.rows("small", F64, p, cus)
    X, y = sc.glm_frame(300 + p, family, n, p, bias)
    bo, it_o = orc.glm_irls(X, y, family, add_bias=bias, tol=1e-10, max_iter=100)
    glm = GLM(add_bias=bias, family=family, max_iter=100, tol=1e-10).fit(torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda())
    b = np.r_[glm.coeffs(), glm.bias()] if bias else glm.coeffs()
    print(f"glm {family} p={p} bias={bias}: {nrel(b, bo):.2e}, iterations {glm.n_iter_} / {it_o}")
    assert nrel(b, bo) < 1e-9 and abs(glm.n_iter_ - it_o) <= 1


@pytest.mark.parametrize("p,family,bias", sc.GLM_F32_CASES)
def test_glm_f32(pds, orc, cus, p, family, bias):
    import torch

    from polars_ds_extension_amd.linear_models import GLM

    n = sc.rows("small", F32, p, cus)
    X, y = sc.glm_frame(400 + p, family, n, p, bias)
    X32, y32 = X.astype(np.float32), y.astype(np.float32)
    bo, _ = orc.glm_irls(X, y, family, add_bias=bias, tol=1e-10, max_iter=100)
    o32, _ = orc.glm_irls(X32, y32, family, add_bias=bias, tol=1e-6, max_iter=100)
    with precision(pds, F32):
        glm = GLM(add_bias=bias, family=family, max_iter=100, tol=1e-6).fit(torch.from_numpy(X32).cuda(), torch.from_numpy(y32).cuda())
    b32 = np.r_[glm.coeffs(), glm.bias()] if bias else glm.coeffs()
    d_gpu, d_orc = nrel(b32, bo), nrel(o32, bo)
    print(f"glm f32 {family} p={p}: gpu-truth {d_gpu:.2e}  orc32-truth {d_orc:.2e}")
    assert d_gpu < 1e-4 or d_gpu <= 1.25 * d_orc


# ------------------------------------------------------------------------------------------ 4. 17 .. 64 features
@functools.lru_cache(maxsize=1)
def _wide_case(p, n):
    X, y, w = sc.wide_report_frame(900 + p, n, p)
    return X, y, w, cols_of(X), dev(y), dev(w)


@pytest.mark.parametrize("se", ["se", "hc1", "hc3", "wls"])
@pytest.mark.parametrize("p", sc.MID_P)
def test_wide_report(pds, orc, cus, p, se):
    """17 .. 64 f64 features: residuals, leverages and the meat out of one moments_mid_kernel<FUSE = 1 / 2> stream (two LDS images,
    half-tile h + 1 in flight while h is consumed); SE and the weighted report through pass2_wide_kernel.  Bars of
    test_gpu_parity.test_wide_weighted_and_hc."""
    bias = p % 2 == 1
    n = sc.rows("mid", F64, p, cus)
    X, y, w, cols, ty, tw = _wide_case(p, n)
    Xb = np.c_[X, np.ones(n)] if bias else X
    if se == "wls":
        r = pds.lin_reg_report(*cols, target=ty, add_bias=bias, weights=tw, y_var=float(np.var(y, ddof=1)))
        ro = orc.wls_report(Xb, y, w)
    else:
        r = pds.lin_reg_report(*cols, target=ty, add_bias=bias, std_err=se)
        ro = orc.lin_reg_report(Xb, y, std_err=se)
    key = "std_err" if se == "wls" else se_key(se)
    e_b, e_s, e_r = nrel(r["beta"], ro["beta"]), frel(r[key], ro["std_err"]), abs(r["r2"][0] - ro["r2"])
    print(f"wide report p={p} {se}: beta {e_b:.2e}  se {e_s:.2e}  r2 {e_r:.2e}")
    assert e_b < F64_TOL and e_s < 1e-9 and e_r < 1e-11


@pytest.mark.parametrize("p", sc.MID_F32_P)
def test_wide_report_f32(pds, orc, cus, p):
    n = sc.rows("mid", F32, p, cus)
    X, y, _ = sc.wide_report_frame(950 + p, n, p)
    X32, y32 = X.astype(np.float32), y.astype(np.float32)
    with precision(pds, F32):
        r = pds.lin_reg_report(*cols_of(X32), target=dev(y32), add_bias=True, std_err="hc3")
    ro32 = orc.lin_reg_report(np.c_[X32, np.ones(n, np.float32)], y32, std_err="hc3")
    ro = orc.lin_reg_report(np.c_[X32.astype(np.float64), np.ones(n)], y32.astype(np.float64), std_err="hc3")
    hold_f32(f"wide report f32 p={p}: hc3", r["hc3_se"], ro32["std_err"], ro["std_err"], frel)
    hold_f32(f"wide report f32 p={p}: beta", r["beta"], ro32["beta"], ro["beta"])


@pytest.mark.parametrize("p,family", sc.MID_GLM_CASES)
def test_wide_glm(pds, orc, cus, p, family):
    """Bars of test_linear_models.test_glm_beyond_16_features_matches_the_oracle (f64 and its f32 rule)."""
    import torch

    from polars_ds_extension_amd.linear_models import GLM

    n = sc.rows("mid", F64, p, cus)
    X, y = sc.wide_glm_frame(11 + p, family, n, p)
    bo, it_o = orc.glm_irls(X, y, family, add_bias=True, tol=1e-10, max_iter=100)
    Xd, yd = torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()
    glm = GLM(add_bias=True, family=family, max_iter=100, tol=1e-10).fit(Xd, yd)
    b = np.r_[glm.coeffs(), glm.bias()]
    print(f"wide glm {family} p={p}: {nrel(b, bo):.2e}, iterations {glm.n_iter_} / {it_o}")
    assert nrel(b, bo) < 1e-9 and abs(glm.n_iter_ - it_o) <= 1
    with precision(pds, F32):
        glm = GLM(add_bias=True, family=family, max_iter=100, tol=1e-6).fit(Xd, yd)
    b32 = np.r_[glm.coeffs(), glm.bias()]
    o32, _ = orc.glm_irls(X.astype(np.float32), y.astype(np.float32), family, add_bias=True, tol=1e-6, max_iter=100)
    d_gpu, d_orc = nrel(b32, bo), nrel(o32, bo)
    print(f"wide glm f32 {family} p={p}: gpu-truth {d_gpu:.2e}  orc32-truth {d_orc:.2e}")
    assert d_gpu < 1e-4 or d_gpu <= 1.25 * d_orc


@pytest.mark.parametrize("p", [20, 40])
def test_wide_pred_steady_state(pds, cus, p):
    """pass2_wide_kernel's grid-stride loop with a second and third trip per lane, through lin_reg(return_pred=True) -- the route to that
    kernel that every build has: pred is the returned coefficients applied to the row (test_grouped_pred's bound), resid = y - pred."""
    n = sc.rows("pass2_wide", F64, p, cus)
    X, y, _ = sc.wide_report_frame(970 + p, n, p)
    cols, ty = cols_of(X), dev(y)
    b = pds.lin_reg(*cols, target=ty, add_bias=True)
    pred, resid = pds.lin_reg(*cols, target=ty, add_bias=True, return_pred=True)
    pred, resid = pred.cpu().numpy(), resid.cpu().numpy()
    Xb = np.c_[X, np.ones(n)]
    scale = np.linalg.norm(Xb, axis=1) * np.linalg.norm(b)
    np.testing.assert_allclose(pred, Xb @ b, rtol=1e-12, atol=1e-12 * np.max(scale))
    assert np.array_equal(resid, y - pred)


# ---- the three-kernel route behind PDS_REPORT_NO_FUSE (read once per process: a fresh interpreter)
def _nofuse_child(out_path):
    import polars_ds_extension_amd as pds

    pds.config.LIN_REG_EXPR_F64 = True
    ctx = pds.default_context()
    ctx.set_timing(True)
    out = {}
    for p in (20, 40):
        n = sc.nofuse_rows(p, ctx.num_cus)
        X, y, _ = sc.wide_report_frame(980 + p, n, p)
        cols, ty = cols_of(X), dev(y)
        for se in ("hc2", "hc3"):
            ctx.get_timing(reset=True)
            r = pds.lin_reg_report(*cols, target=ty, add_bias=True, std_err=se)
            ctx.synchronize()
            t = ctx.get_timing(reset=True)
            out[f"{p}_{se}_beta"], out[f"{p}_{se}_se"], out[f"{p}_{se}_r2"] = r["beta"], r[se_key(se)], np.asarray(r["r2"][:1])
            # launches of the second-pass class: 1 = the fused stream, 2 = pass2_wide_kernel + leverage_mid_kernel
            out[f"{p}_{se}_pass2_launches"] = np.asarray([t["pass2"][1]])
        del cols, ty
    np.savez(out_path, **out)


@pytest.fixture(scope="module")
def nofuse_reports(pds):
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "nofuse.npz")
        env = dict(os.environ, PDS_REPORT_NO_FUSE="1")
        res = subprocess.run([sys.executable, str(Path(__file__).resolve()), out], env=env, timeout=120, capture_output=True, text=True)
        assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
        with np.load(out) as z:
            return {k: z[k] for k in z.files}


@pytest.mark.parametrize("p,se", sc.NOFUSE_CASES)
def test_report_with_the_fusion_switched_off(pds, orc, cus, nofuse_reports, p, se):
    """HC2 / HC3 reports of a fresh interpreter started with PDS_REPORT_NO_FUSE=1, at a row count past the thresholds of both
    pass2_wide_kernel and leverage_mid_kernel, held to the same oracle bars as the fused route.  The switch is a development switch
    (common.hpp dev_env: read only by a library built with -DPDS_DEV_SWITCHES): there the reports come from pass2_wide_kernel +
    leverage_mid_kernel + the weighted Gram build; the default build compiles the fused route in, and the child then repeats it at
    this larger row count.  Which one ran is printed (launches of the second-pass kernel class: 1 fused, 2 un-fused)."""
    n = sc.nofuse_rows(p, cus)
    X, y, _ = sc.wide_report_frame(980 + p, n, p)
    ro = orc.lin_reg_report(np.c_[X, np.ones(n)], y, std_err=se)
    b, s, r2 = nofuse_reports[f"{p}_{se}_beta"], nofuse_reports[f"{p}_{se}_se"], float(nofuse_reports[f"{p}_{se}_r2"][0])
    launches = int(nofuse_reports[f"{p}_{se}_pass2_launches"][0])
    print(f"p={p} {se}: second-pass launches {launches} ({'un-fused' if launches >= 2 else 'fused'}); beta {nrel(b, ro['beta']):.2e}  "
          f"se {frel(s, ro['std_err']):.2e}  r2 {abs(r2 - ro['r2']):.2e}")
    assert nrel(b, ro["beta"]) < F64_TOL and frel(s, ro["std_err"]) < 1e-9 and abs(r2 - ro["r2"]) < 1e-11


# ------------------------------------------------------------------------------------------ 5. grouped_pred_kernel
def _pred_frame(p, dtype, bias, cus):
    """Frame, offsets and group ids on the device (seeded generator)."""
    import torch

    tdt = torch.float64 if dtype == F64 else torch.float32
    n = sc.rows("grouped_pred", dtype, p, cus)
    chunk = sc.unit_rows("grouped_pred", dtype, p)
    wave_chunks = int(sc.units_per_wave("grouped_pred", dtype, p, n, cus).max())
    sizes = sc.pred_group_sizes(500 + p, n, p + int(bias), chunk, wave_chunks)
    g = torch.Generator(device="cuda")
    g.manual_seed(7000 + 10 * p + int(bias))
    st = torch.from_numpy(sizes).cuda()
    off = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.cumsum(st, 0)])
    gid = torch.repeat_interleave(torch.arange(len(sizes), device="cuda"), st)
    cols = [torch.randn(n, generator=g, device="cuda", dtype=torch.float64) for _ in range(p)]
    y = 0.1 * torch.randn(n, generator=g, device="cuda", dtype=torch.float64) + (0.7 if bias else 0.0)
    for j, c in enumerate(cols):
        y += c * (torch.sin(gid.double() * (0.37 + 0.11 * j)) + 0.25 * (-1.0) ** j)  # every group its own coefficients
    return n, sizes, off, gid, [c.to(tdt) for c in cols], y.to(tdt)


@pytest.mark.parametrize("p,dtype,bias", sc.PRED_CASES)
def test_grouped_pred_steady_state(pds, cus, p, dtype, bias):
    """grouped_pred_kernel MODE 0 with 2 .. 3 chunks per wave and MODE 1 (rows shuffled, results sent back through `perm`): the group
    cursor walks forward from chunk to chunk through runs of one-row groups, runs of empty groups, null groups and a group longer than
    a wave's whole range, and the wave's coefficient stage is refilled per chunk (or bypassed).  No oracle: the fits are lin_reg_by's."""
    import torch

    n, sizes, off, gid, cols, ty = _pred_frame(p, dtype, bias, cus)
    pp = p + int(bias)
    with precision(pds, dtype):
        pred, resid, rn, co, nu = pds.lin_reg_by_pred(*cols, target=ty, group_offsets=off, add_bias=bias)
        pred2, resid2, rn2, co2, nu2 = pds.lin_reg_by_pred(*cols, target=ty, group_offsets=off, add_bias=bias)
    rnb, nub = rn.bool(), nu.bool()
    # row_null[r] == is_null[g(r)], pred NaN exactly there; a group below p' rows is null
    assert torch.equal(rnb, nub[gid])
    assert torch.equal(torch.isnan(pred), rnb) and torch.equal(torch.isnan(resid), rnb)
    small = torch.from_numpy(sizes < pp).cuda()
    assert bool(nub[small].all()) and int(small.sum()) > 100 and int((~rnb).sum()) > n // 2
    assert pp == 1 or int(rnb.sum()) > 100  # (p' = 1: only an empty group is too small, and it has no rows)
    ok = ~rnb
    # pred[r] = coeffs[g(r)] . row r (f64 on the device), at test_grouped_pred's bound; f32: the kernel sums in f64 and rounds once
    cg = torch.nan_to_num(co.double())[gid]
    own = cg[:, p].clone() if bias else torch.zeros(n, dtype=torch.float64, device="cuda")
    sq = torch.ones(n, dtype=torch.float64, device="cuda") if bias else torch.zeros(n, dtype=torch.float64, device="cuda")
    for j, c in enumerate(cols):
        own += c.double() * cg[:, j]
        sq += c.double() ** 2
    scale = torch.sqrt(sq) * torch.linalg.norm(cg, dim=1)
    err = (pred.double() - own).abs()[ok]
    bound = 1e-12 * own.abs()[ok] + 1e-12 * float(scale[ok].max())
    if dtype == F32:
        bound = bound + 2.0 ** -24 * own.abs()[ok]  # (one rounding of the f64 sum to f32)
    assert bool((err <= bound).all()), float((err / bound).max())
    # resid = y - pred: one f64 subtraction of the stored prediction, rounded to the frame's precision
    assert torch.equal(resid[ok], (ty.double() - pred.double()).to(ty.dtype)[ok])
    # run to run
    assert torch.equal(pred[ok], pred2[ok]) and torch.equal(resid[ok], resid2[ok]) and torch.equal(rn, rn2)
    assert torch.equal(co[~nub], co2[~nub]) and torch.equal(nu, nu2)
    del pred2, resid2, rn2, co2, cg, own, sq

    # the same frame with its rows shuffled (the order of a group's rows among themselves kept: the stable sort then hands the kernels
    # the ordered frame again), through the sorting route: MODE 1 writes every row's result where the row is
    key = gid * 3 - 1000
    r = torch.rand(n, generator=torch.Generator(device="cuda").manual_seed(99), device="cuda", dtype=torch.float64)
    within = torch.sort(gid.double() + r).values - gid.double()  # ascending inside every group, uniform over the frame
    perm = torch.argsort(within, stable=True)
    ctx = pds.Context(0)
    try:
        ctx.set_option("keyed_sort", 1)
        with precision(pds, dtype):
            ps, rs, ns = pds.lin_reg_by_key_pred(*[c[perm] for c in cols], target=ty[perm], key=key[perm], add_bias=bias, ctx=ctx)
    finally:
        ctx.close()
    assert torch.equal(ns.bool(), rnb[perm])
    okp = ok[perm]
    errp = (ps.double() - pred[perm].double()).abs()[okp]
    boundp = 1e-12 * pred[perm].double().abs()[okp] + 1e-12 * float(scale[ok].max())
    assert bool((errp <= boundp).all()), float((errp / boundp).max())
    errr = (rs.double() - resid[perm].double()).abs()[okp]
    assert bool((errr <= boundp + 1e-12 * resid[perm].double().abs()[okp]).all())
    assert torch.equal(torch.isnan(ps), ~okp)


if __name__ == "__main__":
    _nofuse_child(sys.argv[1])
