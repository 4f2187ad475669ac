"""No GPU: the ABI of batched tracing with sweeps (include/uvrt.h uvrt_trace_batch_launches) -- the symbol in both
libraries, the binding's layout of uvrt_launch against a C compiler's, and the argument check that needs no device."""
import ctypes as C
import os
import subprocess

import numpy as np

from conftest import ROOT


def test_symbol_is_declared_and_resolves_in_both_libraries(pkg):
    assert "uvrt_trace_batch_launches" in [name for name, _, _ in pkg.capi.SYMBOLS]
    for path in (pkg.capi.LIB_PATH, pkg.capi.LIB_DEV_PATH):
        assert hasattr(C.CDLL(path), "uvrt_trace_batch_launches"), path
    for dev in (False, True):
        assert pkg.capi.lib(dev).uvrt_trace_batch_launches.restype is C.c_int


def test_launch_binding_matches_the_header(pkg, tmp_path):
    """uvrt_launch as the Python binding lays it out (capi.LAUNCH_DT) = as a C compiler lays out the struct of
    include/uvrt.h: same size and field offsets; the two kinds are the header's."""
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "uvrt.h"\nint main(void){printf("%zu %zu %zu %zu %zu %d %d\\n",'
                   'sizeof(uvrt_launch), offsetof(uvrt_launch, from), offsetof(uvrt_launch, to),'
                   'offsetof(uvrt_launch, kind), offsetof(uvrt_launch, reserved),'
                   '(int)UVRT_LAUNCH_STOP, (int)UVRT_LAUNCH_SWEEP);return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    dt = pkg.capi.LAUNCH_DT
    want = [dt.itemsize] + [dt.fields[f][1] for f in ("from", "to", "kind", "reserved")] + [pkg.capi.LAUNCH_STOP, pkg.capi.LAUNCH_SWEEP]
    assert got == want and dt.itemsize == 32
    one = np.array([pkg.capi.sweep((1, 2, 3), (4, 5, 6)), pkg.capi.stop((7, 8, 9))], dtype=dt)
    assert one["from"].tolist() == [[1, 2, 3], [7, 8, 9]] and one["to"].tolist() == [[4, 5, 6], [0, 0, 0]]
    assert one["kind"].tolist() == [pkg.capi.LAUNCH_SWEEP, pkg.capi.LAUNCH_STOP] and not one["reserved"].any()


def test_null_context_is_refused_without_a_gpu(pkg):
    launches = np.array([pkg.capi.stop((0, 1, 0))], dtype=pkg.capi.LAUNCH_DT)
    for dev in (False, True):
        L = pkg.capi.lib(dev)
        rc = L.uvrt_trace_batch_launches(None, launches.ctypes.data_as(C.c_void_p), 1.0, 1, 0, 100)
        assert rc == -1 and b"uvrt_trace_batch_launches" in L.uvrt_last_error()          # UVRT_ERR_INVALID
