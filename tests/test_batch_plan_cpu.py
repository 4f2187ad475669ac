"""The host-only plan of a batch (csrc/uvrt_batch_plan.h) without a GPU: tests/tools/batch_plan_check.cpp, alone in a g++
build with stand-ins for the two SEED functions, runs plan_batch over its grid of launch lists, ranges and knobs and holds
every plan to the invariants the emitters of uvrt_capi_batch.hip rely on, and the refusals to their codes."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_batch_plan_invariants(tmp_path):
    """Physical planes, the SEED chain, the pieces' and chunks' partitions (piece sizes within a column differ by at most
    one), scratch sizes, class planes, offsets, refusals."""
    exe = tmp_path / "batch_plan_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I",
                           os.path.join(ROOT, "small-project-uv-robot-ray-tracer_amd", "csrc"),
                           os.path.join(ROOT, "tests", "tools", "batch_plan_check.cpp"), "-o", str(exe)])
    run = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.rstrip().endswith("\n0 breaches"), run.stdout[-4000:]
