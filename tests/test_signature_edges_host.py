"""The inputs of tests/signature_edge_cases.py on the CPU: for every case the torch model of tests/signature_model.py gives the
answer the case states from its construction, the dict-based brute force gives it too where the batch is small, and the layout
the case was built for (which pair indices its run occupies, which item a head lies on) holds in the sorted pair list."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import signature_edge_cases as E  # noqa: E402
import signature_model as S  # noqa: E402

ROOT = os.path.dirname(HERE)
BRUTE_MAX = 300                 # valid windows up to which brute_force runs as well


def _check(case, layout=True):
    """The model (and brute_force on a small batch) against the stated answer; the counts that follow from the token lists
    against the stated counts.  -> (k-mer, protein) of every pair of a token batch, or (None, None)"""
    got = S.derive(case.seq, case.off, case.fn, case.otu, case.minp, case.pur)
    assert got.tobytes() == case.want.tobytes(), case.name
    if case.counts["valid_windows"] <= BRUTE_MAX:
        slow = S.brute_force(case.seq, case.off.tolist(), case.fn.tolist(), case.otu.tolist(), case.minp, case.pur)
        assert slow.tobytes() == case.want.tobytes(), case.name
    assert case.counts["signatures"] == len(case.want) and case.counts["proteins"] == len(case.off) - 1 == len(case.fn)
    if case.tok is None or not layout:
        return None, None
    assert case.counts["valid_windows"] == sum(len(m) for m in case.tok), case.name
    assert case.counts["windows"] == int((np.diff(case.off) - 8).sum()), case.name          # no token protein is shorter than 9
    pk, pp = E.pair_list(case.tok, case.fn, case.otu)
    assert case.counts["pairs"] == pk.size and case.counts["kmers"] == np.unique(pk).size, case.name
    if "token" in case.marks:                                   # the k-mer under test occupies pair indices first .. first + length - 1
        at = np.flatnonzero(pk == case.marks["token"])
        assert at.tolist() == list(range(case.marks["first"], case.marks["first"] + case.marks["length"])), case.name
    if "fn_run" in case.marks:                                  # the fn run under test likewise, inside its k-mer
        at = np.flatnonzero(case.fn[pp] == case.marks["fn_run"])
        assert at.tolist() == list(range(case.marks["first"], case.marks["first"] + case.marks["length"])), case.name
    return pk, pp


def test_the_constants_the_edge_cases_are_built_around():
    csrc = os.path.join(ROOT, "kmergutsjava_amd", "csrc")
    text = {name: open(os.path.join(csrc, name)).read() for name in ("kg_device.hpp", "kg_derive.hpp", "kg_host_derive.hpp")}

    def const(name, var, kind="int"):
        return int(re.search(r"constexpr %s %s = (\d+);" % (kind, var), text[name]).group(1))

    assert const("kg_derive.hpp", "kDeriveChunk") == E.LANE == 16
    for kernel in ("derive_collapse_kernel", "derive_run_sums_kernel"):
        assert re.search(r"__launch_bounds__\(256\) void %s" % kernel, text["kg_derive.hpp"])
        assert re.search(r"hipLaunchKernelGGL\(kg::%s, dim3\(grid_of\(\(\w+ \+ kg::kDeriveChunk - 1\) / kg::kDeriveChunk\)\), dim3\(256\)" % kernel,
                         text["kg_host_derive.hpp"])
    assert 256 * E.LANE == E.WG
    assert const("kg_device.hpp", "kScanThreads") * const("kg_device.hpp", "kScanPerThread") == E.SCAN == 2048
    assert const("kg_device.hpp", "kAaWinPerBlock") == E.BLOCK == 64
    assert const("kg_derive.hpp", "kDeriveBins", "uint32_t") == E.BINS

    def shift_for(width):                                       # Deriver::shift_for
        s = 0
        while ((width - 1) >> s) >= E.BINS:
            s += 1
        return s

    assert "while (((width - 1) >> s) >= kg::kDeriveBins) s++;" in text["kg_host_derive.hpp"]
    assert 1 << shift_for(20 ** 8) == E.BIN0 and 1 << shift_for(E.BIN0) == E.BIN1 and shift_for(E.BIN1) == 0
    assert 1 << shift_for(20 ** 8 - E.LAST_BIN) == E.BIN1       # the clipped last bin is cut into the same pieces
    assert E.TOP == 20 ** 8 - 1 and E.LAST_BIN <= E.TOP - 5000 and E.LAST_BIN + E.BIN0 > 20 ** 8
    assert E.MAXI == 2 ** 31 - 1 and (E.MAXI + 1 << 31 | E.MAXI).bit_length() == 63


def test_the_grids_are_the_ones_stated():
    assert sorted(set(l for l, _ in E.LANE_GRID)) == [0, 1, 15, 16, 17, 4095, 4096, 4097] and len(E.LANE_GRID) == 96
    assert sorted(set(r for _, r in E.LANE_GRID)) == [1, 2, 15, 16, 17, 31, 32, 33, 4095, 4096, 4097, 8192]
    assert E.lane_places(15, 33) == [0, 1, 16, 17, 32]          # pair indices 15, 16, 31, 32 and 47
    assert set(E.REVERSED) < set(E.LANE_GRID)
    assert sorted(at - 2 * which for _, at, which in E.SCAN_HEADS if which == 0) == [2047, 2048, 2049, 4095, 4096, 4097]
    assert len(E.SCAN_HEADS) == 18 and E.RANK_N == (1, 2, 3, 4, 5, 255, 256, 257, 4095, 4096, 4097)
    assert E.PURITY == [(4, 5, 80, True), (3, 4, 80, False), (2, 3, 66, True), (2, 3, 67, False), (1, 1, 100, True)]
    assert E.QUOTIENTS[:6] == [(1, 3), (2, 3), (1, 7), (5, 6), (1, 10), (3, 4099)]
    assert E.SPACE_TOKENS == (0, 1, 2 ** 23 - 1, 2 ** 23, 2 ** 23 + 1, 20 ** 8 - 2, 20 ** 8 - 1)
    assert E.BLOCK_AT == (0, 55, 56, 63, 64, 65, 127, 128) and E.BLOCK_LENGTHS == (8, 9, 72, 73)


# ---- a ----

@pytest.mark.parametrize("lead,run", E.LANE_GRID)
def test_fn_run_sums_at_lane_and_workgroup_borders(lead, run):
    """The run under test occupies pair indices lead .. lead + run - 1 and the padded member is the pair the case names."""
    places = E.lane_places(lead, run)
    assert {0, run - 1} <= set(places) and all((lead + a) % E.LANE in (0, E.LANE - 1) for a in places if a not in (0, run - 1))
    cases = list(E.run_sum_cases(lead, run))
    assert len(cases) == 2 * len(places) + 1 + (min(4, len(places)) if (lead, run) in E.REVERSED else 0)
    for k, case in enumerate(cases):
        pk, pp = _check(case, layout=k < 2 or "reversed" in case.name or "tail 0" in case.name)   # the layout of a (lead, run) once each
        if pk is not None:
            lens = np.diff(case.off)
            assert lens[pp[case.marks["padded"]]] == 9 + run and (lens[pp[case.marks["first"]:case.marks["first"] + run]] >= 9).all()
            assert int(lens[pp[lead:lead + run]].sum()) == 10 * run
        if "inside" in case.name:
            assert case.marks["signature"] == (100 * run >= lead + run + 1) == (len(case.want) == 1)
            if len(case.want):
                assert case.want[0].tolist() == (E.T_RUN, 0, 10, 5, np.float32(run) / np.float32(lead + run + 1))
        else:
            assert case.want[case.want["kmer"] == E.T_RUN].tolist() == [(E.T_RUN, 0, 10, 0, 1.0)]


def test_reversed_protein_order_gives_the_same_answer():
    for lead, run in E.REVERSED:
        at = E.lane_places(lead, run)[0]
        a, b = E.run_sum_case(lead, run, at), E.run_sum_case(lead, run, at, reverse=True)
        assert a.want.tobytes() == b.want.tobytes() and a.counts == b.counts
        assert a.seq != b.seq and sorted(np.diff(a.off)) == sorted(np.diff(b.off))


# ---- b ----

@pytest.mark.parametrize("lead,r", E.LANE_GRID)
def test_collapse_inputs(lead, r):
    """X's run of r equal keys is window items lead .. lead + r - 1, Y's r2 abut it; the pairs are lead + 2 + 3."""
    for r2 in E.COLLAPSE_R2:
        case = E.collapse_case(lead, r, r2)
        pk, pp = _check(case)
        assert case.counts["pairs"] == lead + 2 + 3 and case.counts["valid_windows"] == lead + r + r2 + 3
        assert pp[lead:lead + 2].tolist() == [lead, lead + 1]                       # X, then Y
        assert np.diff(case.off)[lead:lead + 2].tolist() == [9 * r, 9 * r2]
        row = case.want[case.want["kmer"] == E.T_RUN]
        assert row.tolist() == [(E.T_RUN, 0, (9 * r + 9 * r2) // 2, 0, 1.0)]


# ---- c ----

@pytest.mark.parametrize("border,at,which", E.SCAN_HEADS)
def test_run_heads_at_the_scan_chunks(border, at, which):
    case = E.scan_heads_case(border, at, which)
    pk, pp = _check(case)
    first = case.marks["first"]
    assert (pk[:first] == 100 + 3 * np.arange(first)).all() and (pp[:first] == 0).all()
    heads = first + np.flatnonzero(np.diff(case.fn[pp[first:first + 7]], prepend=-7))
    assert heads.tolist()[which] == at and len(heads) == 3 and at in (border - 1, border, border + 1)
    assert len(case.want) == first + 1 + 3 and case.want[first]["functionIndex"] == (2, 5, 9)[which] and case.want[first]["otuIndex"] == 4


@pytest.mark.parametrize("s", E.TIE_SIZES)
@pytest.mark.parametrize("border", E.TIE_BORDERS)
def test_ties_on_a_border(border, s):
    for make, level in ((E.fn_tie_case, "fn"), (E.otu_tie_case, "otu")):
        case = make(border, s)
        pk, pp = _check(case)
        key = (case.fn if level == "fn" else case.otu)[pp]
        assert (key[border - s:border] == key[border - 1]).all() and (key[border:border + s] == key[border]).all()
        assert key[border - 1] < key[border] and pk.size == border + s and (pk[border - s:] == E.T_RUN).all()
        row = case.want[-1].tolist()
        assert row[:4] == ((E.T_RUN, 0, 10, 3) if level == "fn" else (E.T_RUN, 2, 12, 3))


# ---- d ----

@pytest.mark.parametrize("c,n,pur,is_sig", E.PURITY)
def test_purity_bound(c, n, pur, is_sig):
    case, got = E.share_case(c, n, 1, pur)
    _check(case)
    assert got == is_sig == (len(case.want) == 1)


@pytest.mark.parametrize("n,minp,is_sig", E.MIN_PROTEINS)
def test_min_proteins_bound(n, minp, is_sig):
    case, got = E.share_case(n, n, minp, 1)
    _check(case)
    assert got == is_sig == (len(case.want) == 1)


@pytest.mark.parametrize("c,n", E.QUOTIENTS)
def test_quotient(c, n):
    case, is_sig = E.share_case(c, n)
    _check(case)
    assert is_sig == (100 * c >= n)
    if is_sig:
        assert case.want["functionWt"][0] == np.float32(c) / np.float32(n)
        assert abs(float(case.want["functionWt"][0]) - c / n) <= 2.0 ** -24 * c / n     # the correctly rounded quotient


# ---- e ----

@pytest.mark.parametrize("n", E.RANK_N)
def test_rank_width_inputs(n):
    case = E.rank_width_case(n)
    pk, pp = _check(case)
    assert (pp[:n] == np.arange(n)).all() and len(case.want) == n + 1
    assert case.want[0]["functionIndex"] == (0 if n <= 2 else E.MAXI) and case.want[-1]["kmer"] == 2 ** 34 + n - 1 < 20 ** 8


@pytest.mark.parametrize("fn,otu", E.LONE)
def test_one_protein_alone(fn, otu):
    case = E.lone_protein_case(fn, otu)
    _check(case)
    assert len(case.want) == (fn >= 0)


# ---- f ----

def test_pass_plan_inputs():
    cases = list(E.pass_cases()) + [E.over_the_cap_case()[0]]
    assert len(cases) == 12
    for case in cases:
        _check(case)
        if case.passes is not None and case.cap:
            need = -(-case.counts["valid_windows"] // case.cap)
            assert (case.passes == 6 == need) if isinstance(case.passes, int) else (case.passes == ("min", need)), case.name


# ---- g ----

def test_window_block_inputs():
    cases = list(E.window_cases())
    made = {(c.marks["length"], c.marks["at"]): w for c, w in cases}
    for (length, at), w in {(72, 63): True, (72, 64): False, (73, 64): True, (73, 65): False, (8, 0): False, (9, 0): True, (9, 1): False,
                            (136, 128): False, (137, 128): True, (64, 55): True, (64, 56): False, (72, 0): True, (73, 0): True}.items():
        assert made[(length, at)] == w, (length, at)
    for case, is_window in cases:
        _check(case)
        assert len(case.want) == 1 + is_window and case.counts["windows"] == max(case.marks["length"] - 8, 0) + 1
        if is_window:
            assert case.want[0]["avgFromEnd"] == case.marks["length"] - case.marks["at"]
