"""The bounded duration solve without a GPU (include/uvrt.h uvrt_plan_solve_bounded, uvrt_plan_read_classes): the
symbols are bound, the two new structs lie as a C compiler lays them out, and a NULL context is refused before any GPU
call."""
import ctypes

from test_plan_cpu import _c_layout

UVRT_ERR_INVALID = -1      # include/uvrt.h


def test_bounded_solve_symbols_are_bound(pkg):
    L = pkg.capi.lib()
    names = [s[0] for s in pkg.capi.SYMBOLS]
    for name in ("uvrt_plan_solve_bounded", "uvrt_plan_read_classes"):
        assert name in names and getattr(L, name).restype is ctypes.c_int


def test_bounds_structs_match_the_header(pkg, tmp_path):
    for cls, struct in ((pkg.capi.PlanBounds, "uvrt_plan_bounds"), (pkg.capi.PlanBoundsReport, "uvrt_plan_bounds_report")):
        fields = [name for name, _ in cls._fields_]
        got = _c_layout(tmp_path, struct, fields)
        want = [ctypes.sizeof(cls)] + [getattr(cls, f).offset for f in fields]
        assert got == want, (struct, got, want)


def test_null_context_is_refused_without_a_gpu(pkg):
    L = pkg.capi.lib()
    prm, rep, brep = pkg.capi.PlanParams(), pkg.capi.PlanReport(), pkg.capi.PlanBoundsReport()
    out = (ctypes.c_float * 4)()
    cls = (ctypes.c_uint8 * 4)()
    assert L.uvrt_plan_solve_bounded(None, ctypes.byref(prm), None, out, ctypes.byref(rep), ctypes.byref(brep)) == UVRT_ERR_INVALID
    assert L.uvrt_plan_read_classes(None, cls, 0, 4) == UVRT_ERR_INVALID
