"""GPU suite: boundary sweep of the CSR-adaptive walks of the fused hop SpMM -- the binned short list (short_list_blocks), the
medium list (medium_list_blocks), their interleave in groups of 8 workgroups, and the in-tile short-row mode
(in_tile_short_rows); h2gcn_amd/csrc/spmm_kernels.hip.h, work split in launch() (h2gcn_capi.hip).

Every case is built by tests/spmm_driver.py from PRESCRIBED segment lengths and compared BIT FOR BIT with the canonical-tree
oracle (oracle.gcn_layer.gcn_layer_tree / gcn_layer_grad_tree) on NaN-prefilled, guard-banded outputs, forward, hop subsets and
adjoint, each launch twice; the path taken is asserted through plan.schedule / plan.segment_classes.  What each family reaches
is asserted on the CPU by tests/test_spmm_driver.py; the families:

A  class edges: every length around the short / medium / long boundaries and the 64-entry chunks of the medium walk, under
   long_row_threshold 256 / 17 / 16 / 9 / 2 / 1 / 512, at every row position mod 4, first and last in a tile and in row n - 1;
   variants 6 (lists) / 5 (in-tile, rows_per_wave 0 / 1 / 3 / 7: rounds all short, with one row of LPR + 1, with one long row,
   a partial last wave for 3 / 7) / 0, each at widths 64, 128, 128 in 64-column slices, 100 and 20 (masked slices); bf16
   sources at every width (threshold 256); the adjoint on transposed-built hops under the same thresholds and widths, with
   selections of 1..5 hops (5: no lists) and in-tile SUM rounds of 2 / 4 rows (rows_per_wave 3 / 7) that hold a long-owned
   row or a row too wide for a lane group at every position.
B  list counts around a wave (4), a workgroup (16) and a group of 8 workgroups (128) at spw = 4, medium counts around 4 and 32,
   short : medium group ratios n:0, 1:n, 1:1, 1:5, 5:1, 3:2, unequal lists over 2 and 3 hops (an empty list beside one of 257
   entries: the chunk-major padding), the same counts for the adjoint's single list.
C  the per-wave steps: 8*WF - 1 ... 64*WF + 7 listed entries give spw 4 ... 64, medium lists of 2*WF + 1 ... 8*WF + 1 entries
   mpw 2 / 5 / 8, the adjoint with 2 / 3 / 4 hops mpw = 4 and spw >= 8 (WF = kWavesToFill).
D  H2GCN_SHORT_HOP_MAJOR / H2GCN_SHORT_PER_WAVE / H2GCN_MED_PER_WAVE, read once per process: three child processes.
E  colidx / vals as views at element offsets 0 / 1 / 15 / 31 into poisoned buffers, once ending at the buffer's end."""
import os
import subprocess
import sys

import pytest
import torch

import spmm_driver as sd

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    assert not any(os.environ.get(k) for k in sd.KNOBS), "the in-process cases assume the library's own work split"
    return torch.device("cuda:0")


def run_all(cases):
    assert cases
    d = dev()
    for c in cases:
        sd.run_case(c, d, env={})


@pytest.mark.parametrize("variant", [6, 5, 0])
@pytest.mark.parametrize("thr", sd.THRESHOLDS)
def test_class_edges(thr, variant):
    run_all([c for c in sd.family_edges(thr) if c.variant == variant])


@pytest.mark.parametrize("thr", sd.THRESHOLDS)
def test_class_edges_adjoint_selections_of_1_to_5_hops(thr):
    run_all(sd.family_edges_adjoint(thr))


@pytest.mark.parametrize("which", ["fwd", "adj", "hops"])
@pytest.mark.parametrize("d", [64, 128])
def test_list_count_edges(d, which):
    pick = {"fwd": lambda c: c.name.startswith("counts fwd s="), "adj": lambda c: c.name.startswith("counts adj"),
            "hops": lambda c: "per_hop" in c.tags}[which]
    run_all([c for c in sd.family_counts() if c.d == d and pick(c)])


N_STEPS = 10


@pytest.mark.parametrize("i", range(N_STEPS))
def test_per_wave_steps(i):
    cases = sd.family_steps()
    assert len(cases) == N_STEPS
    run_all(cases[i:i + 1])


@pytest.mark.parametrize("off", [0, 1, 15, 31])
def test_views_into_poisoned_buffers(off):
    run_all([c for c in sd.family_views() if c.tags["off"] == off])


def test_once_per_process_knobs_in_child_processes():
    """The hop-major order of the short lists (the short_end[] walk) and the per-wave overrides exist only behind environment
    variables the library reads once: each setting gets a fresh child, one after another, and nothing is started after a failure."""
    dev()
    for knobs in ({"H2GCN_SHORT_HOP_MAJOR": "1", "H2GCN_SHORT_PER_WAVE": "8", "H2GCN_MED_PER_WAVE": "2"}, {"H2GCN_SHORT_HOP_MAJOR": "1"},
                  {"H2GCN_SHORT_PER_WAVE": "64", "H2GCN_MED_PER_WAVE": "8"}):
        r = subprocess.run([sys.executable, "-m", "tests.spmm_driver", "--family", "knobs"], cwd=str(sd.ROOT), env={**os.environ, **knobs},
                           capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, (knobs, r.returncode, r.stdout[-3000:], r.stderr[-2000:])
        assert "cases passed" in r.stdout and "FAIL" not in r.stdout, (knobs, r.stdout[-2000:])
