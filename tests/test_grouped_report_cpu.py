"""Grouped lin_reg_report: the C ABI surface (no GPU needed)."""
import re
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
NEW = ["pds_lin_reg_report_grouped_f64", "pds_lin_reg_report_grouped_f32", "pds_lin_reg_report_by_key_f64",
       "pds_lin_reg_report_by_key_f32", "pds_student_t_sf_device"]


def test_exported_and_declared():
    from polars_ds_extension_amd import _lib

    assert all(n in _lib.EXPORTS for n in NEW)
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in NEW)
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "pds_lstsq.h").read_text(), flags=re.S)
    for n in NEW:  # one `int` declaration each (tests/mock_device/build.py parses them)
        assert len(re.findall(rf"^int\s+{n}\s*\(", text, flags=re.M)) == 1, n


def test_mock_trampolines_parse():
    import sys

    sys.path.insert(0, str(ROOT / "tests" / "mock_device"))
    try:
        import build as mock_build
    finally:
        sys.path.pop(0)
    protos = {name: args for _, name, args in mock_build.prototypes()}
    assert [a for _, a in protos["pds_lin_reg_report_grouped_f64"]] == [
        "ctx", "cols", "n_feat", "n_rows", "group_offsets", "n_groups", "space", "add_bias", "se_type", "y_var", "out"]
    assert [a for _, a in protos["pds_lin_reg_report_by_key_f32"]][-3:] == ["out_keys", "out", "n_groups"]


def test_python_surface():
    import polars_ds_extension_amd as pds

    assert callable(pds.lin_reg_report_by) and callable(pds.lin_reg_report_by_key)
    from polars_ds_extension_amd import _lib

    assert len(_lib.ReportGrouped._fields_) == 9
    d = pds.lstsq._report_grouped_dict({k: (np.zeros((2, 3)), None) for k in pds.lstsq._REPORT_KEYS}
                                       | {"r2": (np.zeros(2), None), "adj_r2": (np.zeros(2), None), "is_null": (np.zeros(2, np.uint8), None)},
                                       2, True, "hc3", None)
    assert d["features"] == ["x1", "x2", "__bias__"] and "hc3_se" in d and d["beta"].shape == (2, 3)
