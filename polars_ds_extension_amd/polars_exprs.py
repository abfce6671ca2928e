"""
Polars expression builders that route through libpds_lstsq_hip.so's `_polars_plugin_*` symbols.

Same call signatures as /root/reference/python/polars_ds/exprs/expr_linear.py (`lin_reg` :105-274 incl. the multi-target
form, `lin_reg_w_rcond` :356-410 (+ `by=` / `lin_reg_w_rcond_by_group`), `lin_reg_report` :561-631, `rolling_lin_reg` :482-558, `recursive_lin_reg` :413-479) plus the key-aware
`lin_reg(..., by=key)` of SURVEY.md 8(b) and `lin_reg_by_group`, the frame-level replacement of `group_by().agg(lin_reg)`,
`logistic_reg` (:277-353) and the grouped GLM fits `logistic_reg(..., by=key)` / `glm_by_group`.
Importing this module needs `polars` (>= 1.4), which is NOT installable in the build image: tests/test_polars_exprs.py runs
every builder end to end with tests/mini_polars standing in for the engine (it implements the documented plugin calling
convention and the per-group evaluation of `group_by().agg()`); against a REAL Polars the module is still unverified.
"""
from __future__ import annotations

from pathlib import Path
from typing import Any, List

from . import config as cfg

PLUGIN_PATH = Path(__file__).resolve().parent / "csrc" / "libpds_lstsq_hip.so"


def _pl():
    import polars as pl  # deferred: keeps the rest of the package importable without polars

    return pl


def _formula(s: Any):
    pl = _pl()
    if isinstance(s, str):
        return pl.sql_expr(s).alias(s)
    if isinstance(s, pl.Series):
        return pl.lit(s)
    if isinstance(s, pl.Expr):
        return s
    if hasattr(s, "__array__"):
        return pl.lit(pl.Series(values=s.__array__()))
    raise ValueError("Input can only be str or polars expression. The str must be valid SQL strings that polars can understand.")


def _plugin(symbol: str, args, kwargs, **flags):
    from polars.plugins import register_plugin_function

    return register_plugin_function(plugin_path=PLUGIN_PATH, function_name=cfg._which_lin_reg(symbol), args=args, kwargs=kwargs,
                                    pass_name_to_apply=True, **flags)


def _dtype():
    pl = _pl()
    return pl.Float64 if cfg.LIN_REG_EXPR_F64 else pl.Float32


MULTI_BY_LIMIT = "grouped multi-target lin_reg: up to 16 feature columns and 15 targets"


def lin_reg(*x, target, add_bias: bool = False, weights=None, return_pred: bool = False, l1_reg: float = 0.0,
            l2_reg: float = 0.0, tol: float = 1e-5, solver: str = "qr", max_iter: int = 200, null_policy: str = "skip",
            positive: bool = False, singular_x_tol: float | None = None, by=None):
    """
    expr_linear.py:105-274.  `by` (an integer key column, any row order, nulls = one group): every group's fit from ONE plugin call.
    With a list `target` of two or more, `by` gives the multi-target fit per group (`pl_lr_multi_by` / `pl_lr_multi_by_pred`: OLS /
    ridge, 1 .. 16 features, up to 15 targets; `l1_reg`, `positive` and `weights` are not part of the multi-target call, as in the
    reference): a Struct {<key>, target_0, target_1, ..} of coefficient lists per group, a group being null in every target field or in
    none; or, with `return_pred`, {target_i_pred, target_i_resid, ..} per input row.
    """
    if singular_x_tol is None:
        singular_x_tol = 1e-12 if cfg.LIN_REG_EXPR_F64 else 1e-6  # expr_linear.py:179-186
    if isinstance(target, list):  # expr_linear.py:188-233
        n_targets = len(target)
        if n_targets == 0:
            raise ValueError("If `target` is a list, it cannot be empty.")
        if n_targets == 1:
            return lin_reg(*x, target=target[0], add_bias=add_bias, weights=weights, return_pred=return_pred, l1_reg=l1_reg,
                           l2_reg=l2_reg, tol=tol, solver=solver, null_policy=null_policy, singular_x_tol=singular_x_tol, by=by)
        dt = _dtype()
        cols = [_formula(t).alias(f"target_{i}").cast(dt) for i, t in enumerate(target)]
        kwargs = {"bias": add_bias, "null_policy": null_policy, "solver": solver, "last_target_idx": n_targets, "l2_reg": l2_reg,
                  "singular_x_tol": singular_x_tol}
        cols.extend(_formula(z) for z in x)
        if by is not None:  # one call fits every group and every target: the keys are ordered once, X'X is factorised once per group
            if len(x) > 16 or n_targets > 15:
                raise NotImplementedError(MULTI_BY_LIMIT)
            if return_pred:
                # Struct{target_i_pred, target_i_resid, ..}, one row per input row in the frame's own order
                return _plugin("pl_lr_multi_by_pred", [_formula(by), *cols], kwargs).alias("lr_pred")
            # Struct{key, target_0: List, target_1: List, ..}, one row per group, keys ascending
            return _plugin("pl_lr_multi_by", [_formula(by), *cols], kwargs, changes_length=True).alias("coeffs_by")
        if return_pred:
            return _plugin("pl_lr_multi_pred", cols, kwargs).alias("lr_pred")
        return _plugin("pl_lr_multi", cols, kwargs, returns_scalar=True).alias("coeffs")
    if max_iter <= 0:
        raise ValueError("Input `max_iter` must be a positive.")
    weighted = weights is not None
    kwargs = {"bias": add_bias, "null_policy": null_policy, "l1_reg": l1_reg, "l2_reg": l2_reg, "solver": solver, "tol": tol,
              "max_iter": max_iter, "weighted": weighted, "positive": positive, "singular_x_tol": singular_x_tol}
    dt = _dtype()
    cols = ([_formula(weights).cast(dt).rechunk()] if weighted else []) + [_formula(target).cast(dt)] + [_formula(z) for z in x]
    if by is not None:  # one call computes every group (integer key column, any row order, nulls = one group)
        if return_pred:
            # Struct{pred, resid}, one row per input row in the frame's own order: what `.over(by)` / `group_by(by).agg(...)`
            # of `lin_reg(..., return_pred=True)` give per group (tests/test_linear_exprs.py:435-474)
            return _plugin("pl_lr_by_pred", [_formula(by), *cols], kwargs).alias("lr_pred")
        # Struct{key, coeffs}, one row per group, keys ascending
        return _plugin("pl_lr_by", [_formula(by), *cols], kwargs, changes_length=True).alias("coeffs_by")
    if return_pred:
        return _plugin("pl_lr_pred", cols, kwargs).alias("lr_pred")
    return _plugin("pl_lr", cols, kwargs, returns_scalar=True).alias("coeffs")


_GID = "__pds_gid"


def _is_integer_key(df, by) -> bool:
    if not isinstance(by, str):
        return False
    try:
        return bool(df.schema[by].is_integer())
    except Exception:
        return False


def _join(left, right, on, how="left"):
    """null keys must meet null keys (Polars' group_by makes them one group): `nulls_equal` (polars >= 1.24), `join_nulls` before"""
    try:
        return left.join(right, on=on, how=how, nulls_equal=True)
    except TypeError:
        return left.join(right, on=on, how=how, join_nulls=True)


def _with_group_ids(df, by):
    """
    Keys of any dtype (strings, dates, several columns, nulls) -> one dense integer id per row: the distinct key rows in order of
    first appearance get ids 0, 1, ... (`unique(maintain_order=True).with_row_index`), joined back onto the frame.  Returns
    (frame with the id column `__pds_gid`, the key table [id, *by]).  A single integer key column does not need this.
    """
    cols = [by] if isinstance(by, str) else list(by)
    # (the plugin returns its key field as Int64 and `with_row_index` makes UInt32: Polars refuses to join the two)
    keys = df.select(cols).unique(maintain_order=True).with_row_index(_GID).with_columns(_pl().col(_GID).cast(_pl().Int64))
    return _join(df, keys, on=cols), keys


def lin_reg_by_group(df, by, *x, target, return_pred: bool = False, **kwargs):
    """
    The replacement for `df.group_by(by).agg(pds.lin_reg(*x, target=...))` on this backend: ONE plugin call over the whole
    frame (`pl_lr_by`: keys in any row order, one fused kernel for every group) instead of one `pl_lr` call per group.
    An expression cannot know that it sits inside a `group_by` -- Polars hands the plugin one group's rows at a time, which
    costs a host-to-device round trip per group and runs BELOW the CPU reference (the coalescing queue of csrc/plugin.cpp
    only softens that) -- so the rewrite is explicit.
    `by`: one key column of any dtype or a list of key columns; null keys form one group, as in Polars.
    Returns a frame with one row per distinct key: columns *by and `coeffs` (a null list where the reference's per-group call
    returns a null list); integer keys come back ascending, other keys in order of first appearance.
    `return_pred=True` (tests/test_linear_exprs.py:435-474): the input frame with `pred` and `resid` columns, row for row.
    A list `target` of two or more fits every target on every group in the same one call (`pl_lr_multi_by`): one list column per
    target (`target_0`, `target_1`, ..) instead of `coeffs`, a null group null in all of them; with `return_pred` the columns
    `target_i_pred` / `target_i_resid`.
    """
    if return_pred:
        if _is_integer_key(df, by):
            return df.with_columns(lin_reg(*x, target=target, by=by, return_pred=True, **kwargs)).unnest("lr_pred")
        ids, _ = _with_group_ids(df, by)
        return ids.with_columns(lin_reg(*x, target=target, by=_GID, return_pred=True, **kwargs)).unnest("lr_pred").drop(_GID)
    if _is_integer_key(df, by):
        # (the key field comes back Int64 under the key column's name: back to the frame's own integer dtype, so that callers
        #  -- lin_reg_over below -- can join it onto the frame)
        res = df.select(lin_reg(*x, target=target, by=by, **kwargs)).unnest("coeffs_by")
        return res.with_columns(_pl().col(by).cast(df.schema[by]))
    ids, keys = _with_group_ids(df, by)
    res = ids.select(lin_reg(*x, target=target, by=_GID, **kwargs)).unnest("coeffs_by")
    return _join(keys, res, on=[_GID]).drop(_GID)


def lin_reg_over(df, by, *x, target, **kwargs):
    """
    `df.with_columns(pds.lin_reg(*x, target=...).over(by))` (examples/basics.ipynb cells 16 / 18): every row carries its group's
    coefficient list.  One `pl_lr_by` call, then the per-group lists are joined back onto the frame.
    """
    cols = [by] if isinstance(by, str) else list(by)
    return _join(df, lin_reg_by_group(df, by, *x, target=target, **kwargs), on=cols)


def lin_reg_w_rcond(*x, target, add_bias: bool = False, rcond: float = 0.0, l2_reg: float = 0.0, null_policy: str = "raise", by=None):
    """
    expr_linear.py:356-410: SVD solve with a singular-value cut-off; Struct{coeffs, singular_values}.
    `by` (an integer key column, any row order, nulls = one group): every group's minimum-norm fit from ONE `pl_lr_w_rcond_by` call --
    Struct{<key>, coeffs, singular_values} per group, keys ascending, null lists for a null group; the cut of a group is
    max(rcond, eps * max(n_g, p')) with the group's own row count.  Keys of other dtypes or several key columns:
    `lin_reg_w_rcond_by_group`.
    """
    cols = [_formula(target).cast(_dtype())] + [_formula(z) for z in x]
    kwargs = {"bias": add_bias, "null_policy": null_policy, "l1_reg": 0.0, "l2_reg": l2_reg, "solver": "", "tol": abs(rcond)}
    if by is not None:
        if len(x) > 16:
            raise NotImplementedError("grouped lin_reg_w_rcond: up to 16 feature columns")
        return _plugin("pl_lr_w_rcond_by", [_formula(by), *cols], kwargs, changes_length=True).alias("rcond_by")
    return _plugin("pl_lr_w_rcond", cols, kwargs)


def lin_reg_w_rcond_by_group(df, by, *x, target, **kwargs):
    """
    The replacement for `df.group_by(by).agg(pds.lin_reg_w_rcond(*x, target=...))` on this backend: ONE plugin call over the whole
    frame (`lin_reg_w_rcond(..., by=)`) instead of one `pl_lr_w_rcond` call per group.  `by`: one key column of any dtype or a list of
    key columns; null keys form one group (`lin_reg_by_group`'s conventions).  Returns a frame with one row per distinct key:
    columns *by, `coeffs` and `singular_values` (null lists for a null group); integer keys come back ascending, other keys in order
    of first appearance.
    """
    if _is_integer_key(df, by):
        res = df.select(lin_reg_w_rcond(*x, target=target, by=by, **kwargs)).unnest("rcond_by")
        return res.with_columns(_pl().col(by).cast(df.schema[by]))
    ids, keys = _with_group_ids(df, by)
    res = ids.select(lin_reg_w_rcond(*x, target=target, by=_GID, **kwargs)).unnest("rcond_by")
    return _join(keys, res, on=[_GID]).drop(_GID)


def lin_reg_report(*x, target, add_bias: bool = False, weights=None, std_err: str = "se", null_policy: str = "raise", by=None,
                   cluster=None, absorb=None, cluster_key=None):
    """
    expr_linear.py:561-631.  `by` (an integer key column, any row order, nulls = one group): every group's report from ONE
    `pl_lin_reg_report_by` / `pl_wls_report_by` call, in long format -- a Struct {<key>, features, beta, <se>, t, p>|t|, 0.025, 0.975,
    r2, adj_r2} with p' rows per group, groups in ascending key order: after `unnest` what
    `group_by(by).agg(lin_reg_report(...)).explode(...)` gives.  var(y) is each group's own.  A group with fewer rows than
    coefficients keeps its rows with null numeric fields.  Keys of other dtypes or several key columns: `lin_reg_report_by_group`.
    `std_err="cluster"` (CR1) / `"cluster0"` (CR0) with `cluster` (an integer key column, any row order, the null key its own
    cluster): ONE model over the whole frame with cluster-robust standard errors from one `pl_lin_reg_report_cluster` call -- the
    Struct of `pl_lin_reg_report` with the standard-error field named `cluster_se` / `cluster0_se`; t, p and the interval use G - 1
    degrees of freedom.  `cluster` together with `by` or `weights` is not implemented.
    `absorb` (an integer key column, any row order, the null key its own group): the fixed-effects regression -- ONE model with an
    intercept per group, the within estimator -- from one `pl_lin_reg_report_within` call.  The Struct of `pl_lin_reg_report` with p
    rows (no `__bias__`: `add_bias=True` is refused); `std_err` is "se" (n - G - p degrees of freedom), "cluster" or "cluster0" --
    the clusters are the absorbed groups, so `cluster` is refused; r2 / adj_r2 are the within values.  `absorb` together with `by`
    or `weights` is not implemented; the effects and the per-row outputs are `lstsq.lin_reg_report(absorb=, ...)` only, and so are
    two absorbed keys (`absorb=[k1, k2]`).  `cluster_key` (errors clustered on a key other than the absorbed one) has no plugin symbol:
    NotImplementedError, `lstsq.lin_reg_report(absorb=, cluster_key=)` on column buffers has it.
    """
    if cluster_key is not None:
        raise NotImplementedError("lin_reg_report: `cluster_key` is not available as an expression; standard errors clustered on any key "
                                  "are `lstsq.lin_reg_report(..., absorb=, cluster_key=)` on column buffers")
    if absorb is not None:
        if isinstance(absorb, (list, tuple)):
            raise NotImplementedError("lin_reg_report: a list of absorbed keys is not available as an expression; two absorbed keys are "
                                      "`lstsq.lin_reg_report(..., absorb=[k1, k2])` on column buffers")
        if add_bias:
            raise ValueError("`add_bias=True` together with `absorb`: the intercept is absorbed by the group effects")
        if cluster is not None:
            raise ValueError('`cluster` together with `absorb`: std_err="cluster" means the absorbed key')
        if std_err not in ("se", "cluster", "cluster0"):
            raise ValueError('`absorb`: std_err is "se", "cluster" or "cluster0"')
        if by is not None or weights is not None:
            raise NotImplementedError("lin_reg_report: `absorb` together with `by` or `weights` is not implemented")
        kwargs = {"bias": False, "null_policy": null_policy, "std_err": std_err, "solver": "qr", "l1_reg": 0.0, "l2_reg": 0.0, "tol": 0.0}
        return _plugin("pl_lin_reg_report_within", [_formula(absorb), _formula(target).cast(_dtype()), *[_formula(z) for z in x]], kwargs,
                       changes_length=True).alias("lin_reg_report")
    if std_err in ("cluster", "cluster0") or cluster is not None:
        if std_err not in ("cluster", "cluster0"):
            raise ValueError('`cluster` goes with std_err="cluster" or "cluster0" only')
        if cluster is None:
            raise ValueError(f'std_err="{std_err}" needs `cluster`, the key column of the clusters')
        if by is not None or weights is not None:
            raise NotImplementedError("lin_reg_report: `cluster` together with `by` or `weights` is not implemented")
    dt = _dtype()
    t = _formula(target).cast(dt)
    kwargs = {"bias": add_bias, "null_policy": null_policy, "std_err": std_err, "solver": "qr", "l1_reg": 0.0, "l2_reg": 0.0, "tol": 0.0}
    feats: List[Any] = [_formula(z) for z in x]
    if cluster is not None:  # (no t.var() input: the library derives it from the target)
        return _plugin("pl_lin_reg_report_cluster", [_formula(cluster), t, *feats], kwargs, changes_length=True).alias("lin_reg_report")
    if by is not None:  # (no t.var() input: in front of a keyed call it would be the frame's variance, not the group's)
        if weights is None:
            return _plugin("pl_lin_reg_report_by", [_formula(by), t, *feats], kwargs, changes_length=True).alias("lin_reg_report")
        return _plugin("pl_wls_report_by", [_formula(by), _formula(weights).cast(dt).rechunk(), t, *feats], kwargs,
                       changes_length=True).alias("lin_reg_report")
    if weights is None:
        return _plugin("pl_lin_reg_report", [t.var(), t, *feats], kwargs, changes_length=True).alias("lin_reg_report")
    return _plugin("pl_wls_report", [_formula(weights).cast(dt).rechunk(), t.var(), t, *feats], kwargs,
                   changes_length=True).alias("lin_reg_report")


def lin_reg_report_by_group(df, by, *x, target, **kwargs):
    """
    The replacement for `df.group_by(by).agg(pds.lin_reg_report(*x, target=...)).explode(...)` on this backend: ONE plugin call over
    the whole frame (`lin_reg_report(..., by=)`) instead of one `pl_lin_reg_report` call per group.  `by`: one key column of any
    dtype or a list of key columns; null keys form one group.  Returns the long frame [*by, features, beta, <se>, t, p>|t|, 0.025,
    0.975, r2, adj_r2] with p' rows per group; integer keys come back ascending, other keys in order of first appearance
    (`lin_reg_by_group`'s conventions).
    """
    if _is_integer_key(df, by):
        res = df.select(lin_reg_report(*x, target=target, by=by, **kwargs)).unnest("lin_reg_report")
        return res.with_columns(_pl().col(by).cast(df.schema[by]))
    ids, keys = _with_group_ids(df, by)
    res = ids.select(lin_reg_report(*x, target=target, by=_GID, **kwargs)).unnest("lin_reg_report")
    return _join(res, keys, on=[_GID]).select([*keys.columns[1:], *res.columns[1:]])


def logistic_reg(*x, target, add_bias: bool = True, l1_reg: float = 0.0, l2_reg: float = 0.0, tol: float = 1e-5, max_iter: int = 200,
                 null_policy: str = "skip", return_pred: bool = False, by=None, weights=None, offset=None):
    """
    expr_linear.py:277-353: `pl_logistic_coeffs` / `pl_logistic_pred` (Float64 only, as there), aliases `__coeffs__` / `__pred__`.
    Deliberate deviation: the reference minimises the mean log loss with L-BFGS from a seeded random start and stops at a gradient
    norm; this backend runs IRLS (binomial family) to the same unpenalised maximum-likelihood point and stops when no coefficient
    moves by `tol`.  Without `by`, `l1_reg` / `l2_reg` > 0 raise rather than return an unpenalised fit.
    `by` (an integer key column, any row order, nulls = one group): one logistic model per group from ONE `pl_glm_by` /
    `pl_glm_by_pred` call with family "binomial" -- Struct{<key>, coeffs, n_iter} per group, keys ascending, or the fitted
    probability of every row.  Keys of other dtypes or several key columns: `glm_by_group`.  With `by`, `l1_reg` / `l2_reg` > 0
    fit every group's penalised model (mean log loss + l2_reg / 2 |beta|^2 + l1_reg |beta|_1 over the features, the bias free).
    `weights` / `offset` (column names or expressions, with `by` only): prior weights and an offset per row, as in `glm_by_group` --
    with the target a success proportion and `weights` its trial count, the fit of the expanded Bernoulli frame.  Without `by` the
    reference's signature stands: the two are refused.
    """
    if max_iter <= 0:
        raise ValueError("Input `max_iter` must be a positive.")
    if by is not None:
        return _glm_by(x, target, by, "binomial", add_bias, abs(tol), max_iter, null_policy, return_pred, l1_reg, l2_reg, weights, offset)
    if weights is not None or offset is not None:
        raise NotImplementedError("logistic_reg: weights= / offset= need by= (one model per group); without by they are not built")
    if l1_reg > 0.0 or l2_reg > 0.0:
        raise NotImplementedError("logistic_reg: l1_reg / l2_reg are not supported on this backend; use GLM(family='binomial', "
                                  "l2_reg=...) or by=")
    from polars.plugins import register_plugin_function

    pl = _pl()
    kwargs = {"bias": add_bias, "null_policy": null_policy, "l1_reg": l1_reg, "l2_reg": l2_reg, "solver": "", "tol": abs(tol),
              "max_iter": max_iter}
    cols = [_formula(target).cast(pl.Float64)] + [_formula(z) for z in x]
    if return_pred:
        return register_plugin_function(plugin_path=PLUGIN_PATH, function_name="pl_logistic_pred", args=cols, kwargs=kwargs,
                                        pass_name_to_apply=True).alias("__pred__")
    return register_plugin_function(plugin_path=PLUGIN_PATH, function_name="pl_logistic_coeffs", args=cols, kwargs=kwargs,
                                    pass_name_to_apply=True).alias("__coeffs__")


def _glm_by(x, target, by, family, add_bias, tol, max_iter, null_policy, return_pred, l1_reg=0.0, l2_reg=0.0, weights=None, offset=None):
    from .linear_models import GLM_FAMILIES

    if family not in GLM_FAMILIES:
        raise NotImplementedError(f"GLM family {family!r}: one of {sorted(GLM_FAMILIES)}")
    if max_iter < 1:
        raise ValueError("`max_iter` must be > 1.")
    kwargs = {"bias": add_bias, "null_policy": null_policy, "family": family, "tol": abs(tol), "max_iter": max_iter}
    if l1_reg > 0.0 or l2_reg > 0.0:  # (absent = 0 in the plugin: an unpenalised call keeps the kwargs it had)
        kwargs.update(l1_reg=max(float(l1_reg), 0.0), l2_reg=max(float(l2_reg), 0.0))
        if weights is not None or offset is not None:
            raise NotImplementedError("grouped GLM: l1_reg / l2_reg together with weights= / offset= is not built")
    # (absent = false in the plugin: a call without the two columns keeps the kwargs and the inputs it had)
    extra = []
    if weights is not None:
        kwargs["has_weights"] = True
        extra.append(_formula(weights).cast(_dtype()))
    if offset is not None:
        kwargs["has_offset"] = True
        extra.append(_formula(offset).cast(_dtype()))
    cols = [_formula(by), *extra, _formula(target).cast(_dtype())] + [_formula(z) for z in x]
    if return_pred:
        return _plugin("pl_glm_by_pred", cols, kwargs).alias("glm_pred")
    return _plugin("pl_glm_by", cols, kwargs, changes_length=True).alias("glm_by")


def glm_by_group(df, by, *x, target, family: str = "gaussian", return_pred: bool = False, add_bias: bool = False, tol: float = 1e-8,
                 max_iter: int = 100, null_policy: str = "raise", l1_reg: float = 0.0, l2_reg: float = 0.0, weights=None, offset=None):
    """
    One GLM per group of a frame (families of `linear_models.GLM_FAMILIES`) from ONE plugin call (`pl_glm_by`: keys in any row
    order, every iteration of a group on chip) -- what fitting `GLM(family=...)` on every group of `df.group_by(by)` computes.
    `by`: one key column of any dtype or a list of key columns; null keys form one group, as in Polars (`lin_reg_by_group`'s
    conventions).  Returns a frame with one row per distinct key: columns *by, `coeffs` (bias last; a null list for a group with
    fewer rows than coefficients or a fit that does not end in finite coefficients) and `n_iter`; integer keys come back ascending,
    other keys in order of first appearance.  `return_pred=True`: the input frame with a `glm_pred` column, row for row.
    `l1_reg` / `l2_reg` > 0: every group's elastic-net penalised fit (`lstsq.glm_by` states the objective).
    `weights` / `offset` (column names or expressions): prior weights and an offset per row, R's `glm(weights=, offset=)`
    (`lstsq.glm_by` states the semantics) -- a Poisson rate is `offset=pl.col("exposure").log()`.  A null in either is an error
    whatever `null_policy`; not together with a penalty.  `glm_pred` is then g^-1(x . beta_group + offset).
    """
    args = (family, add_bias, tol, max_iter, null_policy)
    pen = (l1_reg, l2_reg, weights, offset)
    if return_pred:
        if _is_integer_key(df, by):
            return df.with_columns(_glm_by(x, target, by, *args, True, *pen))
        ids, _ = _with_group_ids(df, by)
        return ids.with_columns(_glm_by(x, target, _GID, *args, True, *pen)).drop(_GID)
    if _is_integer_key(df, by):
        res = df.select(_glm_by(x, target, by, *args, False, *pen)).unnest("glm_by")
        return res.with_columns(_pl().col(by).cast(df.schema[by]))
    ids, keys = _with_group_ids(df, by)
    res = ids.select(_glm_by(x, target, _GID, *args, False, *pen)).unnest("glm_by")
    return _join(keys, res, on=[_GID]).drop(_GID)


def glm_report(*x, target, by=None, family: str = "gaussian", add_bias: bool = False, tol: float = 1e-8, max_iter: int = 100,
               null_policy: str = "raise", weights=None, offset=None, std_err: str = "se", cluster=None):
    """
    The report of one GLM per group from ONE `pl_glm_report_by` call (the GLM twin of `lin_reg_report(..., by=)`): `by` is an
    integer key column in any row order, nulls = one group.  Long format -- a Struct "glm_report" {<key>, features, beta, std_err, z,
    p>|z|, 0.025, 0.975, deviance, null_deviance, dispersion, n_iter} with p' rows per group, groups in ascending key order, the
    per-group fields repeated on a group's rows.  z, p and the interval use the normal distribution for every family (statsmodels'
    `use_t=False`; `lstsq.glm_report_by` states the definitions).  A group with a null report keeps its rows with null numeric
    fields.  Penalised fits have no report.  Keys of other dtypes or several key columns: `glm_report_by_group`.
    `weights` / `offset` (column names or expressions): prior weights and an offset per row (`lstsq.glm_report_by` states the
    weighted definitions; `null_deviance` is null-valued NaN under an offset).  A null in either is an error whatever `null_policy`.
    Without `by`: ONE model over the whole frame with robust standard errors from one `pl_glm_report_robust` call --
    `std_err="hc0"` / `"hc1"`, or `"cluster"` / `"cluster0"` with `cluster` (an integer key column, any row order, the null key its own
    cluster); `lstsq.glm_report` states the definitions.  A Struct "glm_report" of p' rows {features, beta, std_err, z, p>|z|, 0.025,
    0.975, deviance, null_deviance, dispersion, n_iter, n_clusters}; z, p and the interval use the normal distribution, n_clusters
    (0 for the hc kinds) is there for a caller who wants t(G - 1).  Model-based errors of one model (`by=None`, `std_err="se"`) are
    `GLM.fit(report=True)` / `lstsq.glm_report`, not an expression (ValueError); robust errors of per-group reports (`by` with a
    robust kind) are not built (NotImplementedError).
    """
    from .linear_models import GLM_FAMILIES
    from .lstsq import _glm_std_err_check

    _glm_std_err_check("glm_report", std_err, cluster, None)
    if by is not None and std_err != "se":
        raise NotImplementedError("glm_report: robust / clustered errors of per-group reports (`by` with std_err != \"se\") are not built")
    if by is None and std_err == "se":
        raise ValueError('glm_report: `by=None` with std_err="se" is no expression: use GLM.fit(report=True) or lstsq.glm_report')
    if family not in GLM_FAMILIES:
        raise NotImplementedError(f"GLM family {family!r}: one of {sorted(GLM_FAMILIES)}")
    if max_iter < 1:
        raise ValueError("`max_iter` must be > 1.")
    kwargs = {"bias": add_bias, "null_policy": null_policy, "family": family, "tol": abs(tol), "max_iter": max_iter}
    if by is None:
        # (every flag is sent: the symbol is new, there is no older kwargs dict to keep)
        kwargs.update(std_err=std_err, has_cluster=cluster is not None, has_weights=weights is not None, has_offset=offset is not None)
        lead = ([_formula(cluster)] if cluster is not None else []) + [_formula(c).cast(_dtype()) for c in (weights, offset) if c is not None]
        cols = [*lead, _formula(target).cast(_dtype())] + [_formula(z) for z in x]
        return _plugin("pl_glm_report_robust", cols, kwargs, changes_length=True).alias("glm_report")
    extra = []
    if weights is not None:
        kwargs["has_weights"] = True
        extra.append(_formula(weights).cast(_dtype()))
    if offset is not None:
        kwargs["has_offset"] = True
        extra.append(_formula(offset).cast(_dtype()))
    cols = [_formula(by), *extra, _formula(target).cast(_dtype())] + [_formula(z) for z in x]
    return _plugin("pl_glm_report_by", cols, kwargs, changes_length=True).alias("glm_report")


def glm_report_by_group(df, by, *x, target, **kwargs):
    """
    `glm_report(..., by=)` over the whole frame for a key column of any dtype or a list of key columns (null keys form one group):
    the long frame [*by, features, beta, std_err, z, p>|z|, 0.025, 0.975, deviance, null_deviance, dispersion, n_iter] with p' rows per
    group; integer keys come back ascending, other keys in order of first appearance (`lin_reg_report_by_group`'s conventions).
    """
    if _is_integer_key(df, by):
        res = df.select(glm_report(*x, target=target, by=by, **kwargs)).unnest("glm_report")
        return res.with_columns(_pl().col(by).cast(df.schema[by]))
    ids, keys = _with_group_ids(df, by)
    res = ids.select(glm_report(*x, target=target, by=_GID, **kwargs)).unnest("glm_report")
    return _join(res, keys, on=[_GID]).select([*keys.columns[1:], *res.columns[1:]])


def rolling_lin_reg(*x, target, window_size: int, add_bias: bool = False, l2_reg: float = 0.0, min_valid_rows: int | None = None,
                    null_policy: str = "raise", by=None):
    """
    expr_linear.py:482-558.  `by` (an integer key column, any row order, nulls = one group): what `.over(by)` gives -- the same
    Struct{coeffs, pred} per row, in frame order -- from ONE `pl_rolling_lr_by` call instead of one `pl_rolling_lr` call per group.
    Keys of other dtypes or several key columns: `rolling_lin_reg_over`.
    """
    n_features = len(x) + int(add_bias)
    if window_size < 2:
        raise ValueError("`window_size` must be >= 2.")
    if n_features > window_size:
        raise ValueError("# features > window size. Linear regression is not well-defined.")
    min_size = min(n_features, window_size) if min_valid_rows is None else int(min_valid_rows)
    kwargs = {"null_policy": null_policy, "n": window_size, "bias": add_bias, "lambda": abs(l2_reg), "min_size": min_size}
    cols = [_formula(target).cast(_dtype())] + [_formula(z) for z in x]
    if by is not None:
        return _plugin("pl_rolling_lr_by", [_formula(by), *cols], kwargs).alias("rolling_lin_reg")
    return _plugin("pl_rolling_lr", cols, kwargs).alias("rolling_lin_reg")


def recursive_lin_reg(*x, target, start_with: int, add_bias: bool = False, l2_reg: float = 0.0, null_policy: str = "raise", by=None):
    """expr_linear.py:413-479; `by` as in rolling_lin_reg (one `pl_recursive_lr_by` call; other key dtypes: recursive_lin_reg_over)."""
    n_features = len(x) + int(add_bias)
    if start_with < n_features:
        raise ValueError("# features > number of rows for the initial fit.")
    kwargs = {"null_policy": null_policy, "n": start_with, "bias": add_bias, "lambda": abs(l2_reg), "min_size": 0}
    cols = [_formula(target).cast(_dtype())] + [_formula(z) for z in x]
    if by is not None:
        return _plugin("pl_recursive_lr_by", [_formula(by), *cols], kwargs).alias("recursive_lin_reg")
    return _plugin("pl_recursive_lr", cols, kwargs).alias("recursive_lin_reg")


def _dense_ids(df, by):
    """
    One dense Int64 id per row for keys of any dtype or several columns (null keys: one group, as in Polars), IN THE FRAME'S ROW
    ORDER: the ids are built on the host from the key rows themselves, without a join, so no engine's join order can move a row.
    """
    cols = [by] if isinstance(by, str) else list(by)
    import numpy as np

    seen: dict = {}
    rows = zip(*[df[c].to_list() for c in cols])
    return _pl().Series(_GID, np.fromiter((seen.setdefault(k, len(seen)) for k in rows), dtype=np.int64, count=len(df)))


def _windowed_over(fn, df, by, x, target, kwargs):
    if _is_integer_key(df, by):
        return df.with_columns(fn(*x, target=target, by=by, **kwargs))
    ids = _dense_ids(df, by)
    return df.with_columns(fn(*x, target=target, by=ids, **kwargs))


def rolling_lin_reg_over(df, by, *x, target, **kwargs):
    """
    `df.with_columns(pds.rolling_lin_reg(*x, target=...).over(by))` in one plugin call, for a key of any dtype or several key
    columns (null keys form one group): the frame with a `rolling_lin_reg` Struct{coeffs, pred} column, row for row.
    """
    return _windowed_over(rolling_lin_reg, df, by, x, target, kwargs)


def recursive_lin_reg_over(df, by, *x, target, **kwargs):
    """`df.with_columns(pds.recursive_lin_reg(*x, target=...).over(by))` in one plugin call (see rolling_lin_reg_over)."""
    return _windowed_over(recursive_lin_reg, df, by, x, target, kwargs)


def query_ar_coeffs(x, lag: int, add_bias: bool = True, null_policy: str = "raise"):
    """exprs/ts_features.py:419-461: AR(lag) coefficients = lin_reg on shifted slices of the one series, bias last."""
    if null_policy not in ("raise", "one", "zero"):
        import math

        try:
            if not math.isfinite(float(null_policy)):
                raise ValueError
        except (TypeError, ValueError):
            raise ValueError("`null_polocy` must be 'raise', 'one', 'zero' or any finite numeric string for AR coefficients.") from None
    if lag <= 0:
        raise ValueError("`lag` must be > 0.")
    pl = _pl()
    xx = pl.col(x) if isinstance(x, str) else x
    return lin_reg(*[xx.shift(i).slice(offset=lag).alias(str(i)) for i in range(1, lag + 1)], target=xx.slice(offset=lag),
                   add_bias=add_bias, null_policy=null_policy)
