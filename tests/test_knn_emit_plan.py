"""Where the emitting int8 scan puts its entries (reindexer_amd/csrc/knn_emit_plan.h), pinned on the CPU by the stand-alone program
tests/cpp/knn_emit_plan_cpu.cc: for every n in 1 .. 70 000 and the grids scan_i8_grid_x gives for 1, 2 and 8 workgroups per CU at 256 CUs the
program deals the sets of 16 rows to the wavefronts one by one and holds the header against that - the segments are disjoint, lie back to
back and hold every row their wavefront scans - and it checks the sizes at n = 2^32 - 1, where anything computed in 32 bits wraps."""
import subprocess
from pathlib import Path

EXE = Path(__file__).resolve().parent / "cpp" / "knn_emit_plan_cpu"


def test_segments_are_disjoint_and_hold_what_their_wavefront_scans():
    if not EXE.exists():
        from reindexer_amd import build
        build.build_cpp_tests()
    r = subprocess.run([str(EXE)], capture_output=True, text=True)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "ok (n up to 70000, 0 failures)" in r.stdout
