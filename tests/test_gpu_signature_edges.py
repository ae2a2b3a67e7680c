"""kg_signatures_derive on its internal borders (kg_derive.hpp, kg_host_derive.hpp): fn runs and equal-key runs against the 16
items of a lane and the 4096 of a workgroup, run heads and ties against the prefix sums' 2048-item chunks, the rank width at
n_prot = 1, 2^k and 2^k +- 1 with 63-bit rank keys, the pass plan (refined bins, one-k-mer passes, a count equal to the cap, the
last partial bin) and the 64-window blocks.

The inputs and their answers come from tests/signature_edge_cases.py, where the answers are stated from the construction;
tests/test_signature_edges_host.py checks the model against them on the CPU.  Here the device's records must equal the model's and
the stated answer byte for byte, and its counts the constructed ones; the first input of every test goes through the device
entry point as well."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import signature_edge_cases as E  # noqa: E402
import signature_model as S  # noqa: E402

from kmergutsjava_amd import _native as N  # noqa: E402

pytestmark = pytest.mark.gpu


def _derive(case, entry="host", cap=0):
    from kmergutsjava_amd import hotpath
    kw = dict(min_proteins=case.minp, purity_pct=case.pur, max_windows_per_pass=cap)
    if entry == "device":
        d = torch.from_numpy(np.frombuffer(case.seq, dtype=np.uint8).copy()).cuda()
        with hotpath.derive_signatures(None, case.off, case.fn, case.otu, device_ptr=d.data_ptr(), **kw) as s:
            return s.numpy(), s.stats()
    with hotpath.derive_signatures(case.seq, case.off, case.fn, case.otu, **kw) as s:
        return s.numpy(), s.stats()


def _check(case, device=False):
    """The host entry point (and the device one) under the case's cap against the model and against the stated answer, the six
    counts against the constructed ones.  -> (records, statistics)"""
    model = S.derive(case.seq, case.off, case.fn, case.otu, case.minp, case.pur)
    for entry in ("host", "device") if device else ("host",):
        got, st = _derive(case, entry, case.cap)
        what = "%s (%s entry)" % (case.name, entry)
        assert got.tobytes() == model.tobytes(), what
        assert got.tobytes() == case.want.tobytes(), what
        assert {k: st[k] for k in E.COUNTS} == case.counts, what
        if case.passes is None:
            assert st["passes"] == (1 if case.counts["valid_windows"] else 0), what
        elif isinstance(case.passes, int):
            assert st["passes"] == case.passes, what
        else:
            assert st["passes"] >= case.passes[1], what
    return got, st


# ---- a. fn-run sums against lane and workgroup borders ------------------------------------------------------------------------

@pytest.mark.parametrize("lead,run", E.LANE_GRID)
def test_fn_run_sums_at_lane_and_workgroup_borders(lead, run):
    """The fn run under test is pair indices lead .. lead + run - 1, as a k-mer of its own (three proteins of the largest token
    behind it, or nothing: the run then ends at end == n) and as the middle fn run of one k-mer.  One member is 9 + run long and
    lies on the first pair, the last, and the pairs 16 k - 1 and 16 k (4096 k - 1 and 4096 k in the long runs): avgFromEnd = 10
    exactly.  Inside a k-mer f* = 5, c = run, n_v = lead + run + 1, and no signature where 100 run < n_v."""
    for k, case in enumerate(E.run_sum_cases(lead, run)):
        got, _ = _check(case, device=k < 2)
        if "inside" in case.name:
            assert len(got) == (100 * run >= lead + run + 1), case.name
        if len(got) and "inside" in case.name:
            assert got[0]["avgFromEnd"] == 10 and got[0]["functionWt"] == np.float32(run) / np.float32(lead + run + 1), case.name


# ---- b. equal keys against lane and workgroup borders -------------------------------------------------------------------------

@pytest.mark.parametrize("lead,r", E.LANE_GRID)
def test_equal_key_runs_at_lane_and_workgroup_borders(lead, r):
    """Protein X's r equal keys are window items lead .. lead + r - 1 and protein Y's 1 or 17 abut them: pairs = lead + 2 + 3 and
    the k-mer's avgFromEnd is floor((9 r + 9 r2) / 2).  The order inside an equal-key run is the emission's and not fixed: the
    case fixes where the run lies, not where its largest value lies."""
    for k, r2 in enumerate(E.COLLAPSE_R2):
        got, st = _check(E.collapse_case(lead, r, r2), device=k == 0)
        assert st["pairs"] == lead + 5 and st["valid_windows"] == lead + r + r2 + 3


# ---- c. run numbers across the scan chunks ------------------------------------------------------------------------------------

@pytest.mark.parametrize("border,at,which", E.SCAN_HEADS)
def test_run_heads_at_the_scan_chunks(border, at, which):
    """at - 2 which distinct k-mers of one protein, every one a k-mer run, an fn run, an OTU run and a signature, then a k-mer of
    three fn runs: the head of fn run `which` is item `at` = 2047 .. 2049 or 4095 .. 4097, and that run is f*.  at + 4 - 2 which
    records."""
    case = E.scan_heads_case(border, at, which)
    got, st = _check(case, device=True)
    assert got[at - 2 * which]["functionIndex"] == (2, 5, 9)[which] and st["signatures"] == at - 2 * which + 4


@pytest.mark.parametrize("s", E.TIE_SIZES)
@pytest.mark.parametrize("border", E.TIE_BORDERS)
def test_ties_on_a_border(border, s):
    """Two fn runs of s proteins on items border - s .. border - 1 and border .. border + s - 1 (border 16, 2048, 4096): the
    smaller f, with its own sum.  Two OTU runs of s inside f* likewise: the smaller OTU."""
    got, _ = _check(E.fn_tie_case(border, s), device=True)
    assert got[-1].tolist()[1:4] == (0, 10, 3)
    got, _ = _check(E.otu_tie_case(border, s))
    assert got[-1].tolist()[1:4] == (2, 12, 3)


# ---- d. thresholds and the quotient -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c,n,pur,is_sig", E.PURITY)
def test_purity_bound(c, n, pur, is_sig):
    """100 c >= purity_pct n, at equality and one below."""
    case, _ = E.share_case(c, n, 1, pur)
    got, _ = _check(case, device=True)
    assert len(got) == is_sig


@pytest.mark.parametrize("n,minp,is_sig", E.MIN_PROTEINS)
def test_min_proteins_bound(n, minp, is_sig):
    """min_proteins = n_v and n_v + 1."""
    got, _ = _check(E.share_case(n, n, minp, 1)[0])
    assert len(got) == is_sig


@pytest.mark.parametrize("c,n", E.QUOTIENTS)
def test_function_weight_is_the_float32_quotient(c, n):
    """functionWt against numpy's float32 division.  (3, 4099) is under purity_pct = 1 and so by rule absent; (41, 4099) has the
    same n_v."""
    got, _ = _check(E.share_case(c, n)[0])
    assert len(got) == (100 * c >= n)
    if len(got):
        assert got["functionWt"][0] == np.float32(c) / np.float32(n)


# ---- e. the rank width --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", E.RANK_N)
def test_rank_width_edges(n):
    """b = ceil(log2 n) at n = 1 (b = 0), 2^k and 2^k +- 1, with fn = otu = 2^31 - 1 on every protein but the first: 63-bit rank
    keys, ~otu packed from the largest OTU.  At n = 2 the k-mer's two functions tie and 0 wins."""
    got, st = _check(E.rank_width_case(n), device=True)
    assert got[0].tolist()[:4] == ((7, 0, 18, 0) if n <= 2 else (7, E.MAXI, got[0]["avgFromEnd"], E.MAXI))


@pytest.mark.parametrize("fn,otu", E.LONE)
def test_one_protein_alone(fn, otu):
    got, st = _check(E.lone_protein_case(fn, otu), device=True)
    assert len(got) == (fn >= 0) and st["passes"] == 1


# ---- f. the k-mer space and the pass plan -------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pass_cases():
    return {c.name: c for c in E.pass_cases()}


PASS_NAMES = [c.name for c in E.pass_cases()]


@pytest.mark.parametrize("name", PASS_NAMES)
def test_pass_plan(pass_cases, name):
    """Under its cap every input gives the bytes of one pass, the model's and the stated ones: the ends of the k-mer space and of
    the first top-level bin; k-mers either side of 2^32, 2^33 and 2^34, the top bits of the one pass's key; six k-mers that are a pass each, their count equal to the cap (with one protein a sort of 0 bits);
    a top-level bin refined into BIN1 pieces, a BIN1 piece refined into single k-mers, and the same in the last top-level bin,
    which 20^8 clips."""
    case = pass_cases[name]
    got, st = _check(case, device=True)
    if case.cap:
        one, st1 = _derive(case)
        assert st1["passes"] == 1 and one.tobytes() == got.tobytes()
        assert st["passes"] >= -(-st["valid_windows"] // case.cap)


def test_one_kmer_over_the_cap_is_named():
    case, text = E.over_the_cap_case()
    for entry in ("host", "device"):
        with pytest.raises(N.KmerGutsNativeError) as ei:
            _derive(case, entry, case.cap)
        assert ei.value.code == N.KG_ERR_LIMIT and text in str(ei.value) and "max_windows_per_pass = 2" in str(ei.value)
    _check(case._replace(cap=3, passes=6))


# ---- g. window blocks ---------------------------------------------------------------------------------------------------------

def test_windows_at_block_edges():
    """A k-mer on window 0, 55, 56, 63, 64, 65, 127 and 128 of a protein gives avgFromEnd = len - i; as the last window
    (i = len - 9) it counts, as the protein's end (i = len - 8) it is no window; lengths 8, 9, 72 and 73."""
    for k, (case, is_window) in enumerate(E.window_cases()):
        got, st = _check(case, device=k % 4 == 0)
        assert len(got) == 1 + is_window and st["valid_windows"] == 1 + is_window, case.name
        if is_window:
            assert got[0]["avgFromEnd"] == case.marks["length"] - case.marks["at"], case.name
