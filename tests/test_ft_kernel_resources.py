"""CPU: build-time resource check of the dense ft_fast train's kernels (reindexer_amd/csrc/ft_ranges.hip, ft_admit.hip, ft_finish.hip,
ft_transfer.hip), after tests/test_knn_tail_resources.py.

hipcc cross-compiles gfx950 without a GPU and `-Rpass-analysis=kernel-resource-usage` prints what the code object header will say.  The
kernels' comments design for a number of workgroups per CU — ft_ranges (about 30 KB of LDS) and ft_rank_all five, ft_finish four (32 KB in
its compact layout): with Q queries in one grid their throughput is that number, so the remark's occupancy (wavefronts per SIMD; a
workgroup of 256 threads puts one on each of the four SIMDs) may not fall below it.  None of the thirteen kernels may use scratch or spill a
vector register: they are chains of dependent phases, and a spill would put memory round trips into every one."""
import shutil
from pathlib import Path

import pytest

from tests.test_range_i8_resources import resource_usage

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "reindexer_amd" / "csrc"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# unit -> its kernels (Itanium names: rxgpu::<kernel>(...)) with the least occupancy each may report
UNITS = {
    "ft_ranges.hip": {"ft_syn_masks": 1, "ft_ranges": 5, "ft_preselect_apply": 1},
    "ft_admit.hip": {"ft_rank_all": 5, "ft_adders": 1, "ft_slot_bases": 1},
    "ft_finish.hip": {"ft_finish": 4},
    "ft_transfer.hip": {"ft_import": 1, "ft_import_pieces": 1, "ft_export": 1, "ft_shard_fold": 1, "ft_shard_hist_combine": 1, "ft_shard_table_sum": 1},
}


@pytest.mark.skipif(not Path(HIPCC).exists(), reason="needs hipcc")
@pytest.mark.parametrize("unit", sorted(UNITS))
def test_ft_kernels_stay_in_registers_and_keep_their_occupancy(unit, tmp_path):
    usage = resource_usage(CSRC / unit, tmp_path)
    found = {}
    for kernel, least in UNITS[unit].items():
        names = [n for n in usage if n.startswith(f"_ZN5rxgpu{len(kernel)}{kernel}E")]
        assert len(names) == 1, (kernel, sorted(usage))
        u = usage[names[0]]
        found[names[0]] = u
        print(f"{kernel}: {u['VGPRs']} VGPRs, occupancy {u['Occupancy']}, {u['LDS Size']} bytes of static LDS, scratch {u['ScratchSize']}")
        assert u["VGPRs Spill"] == 0 and u["ScratchSize"] == 0, (kernel, u)
        assert u["Occupancy"] >= least, (kernel, u["Occupancy"], least)
    assert set(found) == set(usage), sorted(set(usage) - set(found))   # every kernel of the unit is named above


def test_the_train_has_thirteen_kernels():
    assert sum(len(k) for k in UNITS.values()) == 13
