"""kg_assign_calls / kg_result_assign on their internal borders (kg_assign.hpp, kg_host_assign.hpp): the split between the one-lane
path and the sorted path at 16 CALLs, the run walk's blocks of 16 and its guard at the array's end, the wave's merge of the top
two, the sort's key widths, buffer parity and tiles, the second trip of the grid stride, the prefix sum's 2048-item chunk, the
2^31 limit and the thresholds at their bounds on both paths, call_start[0] > 0, and the long path behind a real scan.

The inputs and their answers come from tests/assign_edge_cases.py, where the answers are written down from the construction;
tests/test_assign_edges_host.py checks both forms of the model against them on the CPU.  Here every input goes through
kg_assign_calls with a host and with a device destination, and the records must equal the model's and the case's answer, byte
for byte."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import assign_edge_cases as E  # noqa: E402
import assign_model as A  # noqa: E402
import test_assign_edges_host as H  # noqa: E402
from test_gpu_assign import _dev, _table, strategy  # noqa: E402,F401

from kmergutsjava_amd import _native as N  # noqa: E402

pytestmark = pytest.mark.gpu


def _diff(got, want):
    bad = np.flatnonzero(got != want)
    return "" if not bad.size else "%d records differ, the first at protein %d: got %s, want %s" % (bad.size, bad[0], got[bad[0]], want[bad[0]])


def _check(case, what=""):
    """Host and device destination against the model and the case's answer.  -> the records"""
    calls, cs, otu, (ms, share), answer = case
    want = A.assign(calls, cs, otu, ms, share)
    assert want.tobytes() == answer.tobytes(), what
    for dst in ("host", "device"):
        got = _dev(calls, cs, otu, ms, share, dst)
        assert got.tobytes() == answer.tobytes(), (what, dst, _diff(got, answer))
    return got


# ---- a. path independence at the split ------------------------------------------------------------------------------------------

def test_padded_lists_do_not_depend_on_the_path():
    """200 random lists of 1 to 16 CALLs, each also padded with zero CALLs to 16, 17, 18, 64 and 65, behind and in front: the
    one-lane path and the sorted path must give the list's own record."""
    case, source = E.split_case()
    got = _check(case)
    fields = [f for f in N.ASSIGNMENT_DTYPE.names if f != "n_calls"]
    assert (got[fields] == got[np.searchsorted(source, source)][fields]).all()


# ---- b. rank grid for the merge ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", E.GRID_MODES)
def test_top_two_at_chosen_lanes(mode):
    """The best and the runner-up at every ordered pair of ranks from {0, 1, 31, 32, 63, 64, 65, 127, 128, 129} of 130 one-CALL
    functions (lane = rank % 64), decided by S (1), by W (2), by f (3, 4), and the runner-up by f below a unique best (5); the
    same on the one-lane path with 16 functions."""
    _check(E.grid_case(mode))


# ---- c. the walk --------------------------------------------------------------------------------------------------------------------

def test_runs_inside_the_sorted_array():
    """Runs of 1 .. 257 CALLs, contiguous and interleaved in emission order, 2^24 first and last."""
    _check(E.walk_inner_case())


@pytest.mark.parametrize("arrangement", ["last", "behind"])
def test_runs_at_the_end_of_the_sorted_array(arrangement):
    """The run ends on the sorted array's last item, or 1 to 15 items before it: the walk's block reaches past the array."""
    for L in E.WALK_L:
        for order in E.WALK_ORDERS:
            _check(E.walk_end_case(L, order, arrangement), (L, order))


def test_neighbouring_proteins_of_one_function():
    for lengths in E.NEIGHBOURS + (sum(E.NEIGHBOURS, ()),):
        got = _check(E.neighbours_case(lengths), lengths)
        assert got["score"][::2].tolist() == list(lengths)


# ---- d. the sort's tiles ------------------------------------------------------------------------------------------------------------

def test_one_function_across_the_sort_tiles():
    got = _check(E.tiles_case())
    assert got["weighted"][0] == np.float32(2 ** 24) and got["score"][0] == 6


# ---- e. key widths, buffer parity and the second grid trip ------------------------------------------------------------------------------

@pytest.mark.parametrize("n_long", E.KEY_WIDTH_N_LONG)
def test_key_widths_and_grid_trips(n_long):
    """32 .. 49 key bits in 4 .. 7 passes (the sorted pairs end in either buffer); 65537 long proteins take the grid stride's
    second trip."""
    got = _check(E.key_width_case(n_long))
    assert (got["n_calls"] == 17).sum() == n_long


# ---- f. the prefix sum's chunk ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", E.CHUNK_VARIANTS)
def test_long_proteins_at_the_scan_chunk(variant):
    _check(E.chunk_case(variant))


# ---- g. the 2^31 limit ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("share", [100, 50])
def test_totals_just_below_the_limit(share):
    got = _check(E.below_limit_case(share))
    assert got["total"].tolist() == [2 ** 31 - 1] * 4 and got["assigned"].tolist() == ([1, 0, 1, 0] if share == 100 else [1, 1, 1, 1])


def test_the_limit_names_the_first_protein_on_either_path():
    for name, calls, cs, at in E.limit_error_cases():
        for dst in ("host", "device"):
            with pytest.raises(N.KmerGutsNativeError) as ei:
                _dev(calls, cs, dst=dst)
            assert ei.value.code == N.KG_ERR_LIMIT and ("protein %d:" % at) in str(ei.value), (name, dst, str(ei.value))


# ---- h. thresholds ----------------------------------------------------------------------------------------------------------------------

def test_thresholds_at_their_bound():
    for name, case, ok in E.threshold_cases():
        got = _check(case, name)
        assert got["assigned"].tolist() == [ok, ok], name


# ---- i. call_start[0] = 5 ---------------------------------------------------------------------------------------------------------------

def test_records_in_front_of_the_first_protein():
    for name, case in E.shifted_cases():
        _check(case, name)


# ---- j. behind a scan -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("oc", [False, True])
def test_long_proteins_behind_a_scan(oracle, strategy, oc):
    """Two chimeric proteins whose scan emits more CALLs than one lane takes: kg_result_assign on the scan's own device records
    against the model on the oracle's."""
    from kmergutsjava_amd import hotpath
    train, (qseq, qoff), chimeras = E.scan_inputs()
    img, tab = _table(*train)
    sb = np.frombuffer(qseq, dtype=np.uint8)
    ora = oracle.run(img, sb, qoff, aa=True, lookup_mode=1, order_constraint=oc)
    H.check_scan_records(ora, chimeras, oc)
    with tab:
        live0 = tab.live_device_bytes()
        with tab.scan(sb, qoff, hotpath.Params(aa=True, order_constraint=oc)) as r:
            live1 = tab.live_device_bytes()
            for ms, share in ((0, 50), (10, 80), (0, 0)):
                want = A.assign(ora["calls"], ora["container_call_start"], ora["otu"], ms, share)
                got = r.assign(ms, share)
                assert got.tobytes() == want.tobytes(), _diff(got, want)
                d = r.assign(ms, share, device_out=True)
                assert d.cpu().numpy().tobytes() == want.tobytes()
                assert tab.live_device_bytes() == live1
            assert (got["n_calls"][list(chimeras)] > E.SHORT).all() and got["n_calls"][chimeras[0] + 1] == 0
        assert tab.live_device_bytes() == live0
