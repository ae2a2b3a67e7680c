"""The host side of building a signature table (no GPU): the signature record layout, the text format of
`python -m kmergutsjava_amd.make_table` and its default table size."""
import random

import numpy as np
import pytest


def test_signature_dtype_is_a_table_record():
    from kmergutsjava_amd import _native as N
    d = N.SIGNATURE_DTYPE
    assert d.itemsize == 24
    assert [d.fields[f][1] for f in d.names] == [0, 8, 12, 16, 20]
    assert [d.fields[f][0].str for f in d.names] == ["<i8", "<i4", "<i4", "<i4", "<f4"]


def test_kmer_letters_round_trip_with_decode_kmer():
    from kmergutsjava_amd import make_table as M, synth
    rng = random.Random(7)
    vals = [0, synth.MAX_ENCODED - 1] + [rng.randrange(synth.MAX_ENCODED) for _ in range(2000)]
    text = "".join("%s\t%d\t%d\t%d\t%s\n" % (synth.decode_kmer(v), i % 64, i % 500, i % 1000, (1 + i % 64) / 16)
                   for i, v in enumerate(vals))
    sig = M.parse_signatures(text.encode())
    assert sig["kmer"].tolist() == vals
    assert sig["otuIndex"].tolist() == [i % 64 for i in range(len(vals))]
    assert sig["avgFromEnd"].tolist() == [i % 500 for i in range(len(vals))]
    assert sig["functionIndex"].tolist() == [i % 1000 for i in range(len(vals))]
    assert sig["functionWt"].tolist() == [(1 + i % 64) / 16 for i in range(len(vals))]
    assert [M.kmer_letters(v) for v in vals] == [synth.decode_kmer(v) for v in vals]
    letters = np.frombuffer("".join(synth.decode_kmer(v) for v in vals).encode(), dtype=np.uint8).reshape(-1, 8)
    assert M.encode_kmers(letters).tolist() == vals


def test_blank_lines_and_crlf_are_accepted():
    from kmergutsjava_amd import make_table as M
    sig = M.parse_signatures(b"\nAAAAAAAC\t1\t2\t3\t0.5\r\n  \t\n\nYYYYYYYY\t-4\t5\t6\t2")
    assert sig["kmer"].tolist() == [1, 20 ** 8 - 1]
    assert sig["otuIndex"].tolist() == [1, -4] and sig["functionWt"].tolist() == [0.5, 2.0]
    assert len(M.parse_signatures(b"")) == 0 and len(M.parse_signatures(b"\n\n")) == 0


@pytest.mark.parametrize("text, line, what", [
    ("AAAAAAAA\t1\t2\t3\t0.5\n\nAAAAAABA\t1\t2\t3\t0.5\n", 3, "letter"),      # B is not an amino-acid letter here
    ("AAAAAAAA\t1\t2\t3\t0.5\nAAAAAAAa\t1\t2\t3\t0.5\n", 2, "letter"),
    ("AAAAAAAA\t1\t2\t3\n", 1, "fields"),
    ("AAAAAAAA\t1\t2\t3\t4\t5\n", 1, "fields"),
    ("AAAAAAAA 1 2 3 4\n", 1, "fields"),
    ("AAAAAAAA\t1\t2\t3\t1\nAAAAAAA\t1\t2\t3\t1\n", 2, "8 letters"),
    ("AAAAAAAA\t1\t2\t3\t1\nCCCCCCCC\t1\tx\t3\t1\n", 2, "avgFromEnd"),
    ("\n\nAAAAAAAA\t1.5\t2\t3\t1\n", 3, "otuIndex"),
    ("AAAAAAAA\t1\t2\t\t1\n", 1, "functionIndex"),
    ("AAAAAAAA\t1\t2\t3\t1\nCCCCCCCC\t1\t2\t3\tabc\n", 2, "functionWt"),
    ("AAAAAAAA\t1\t2\t3\t1\nCCCCCCCC\t1\t2\t4294967296\t1\n", 2, "32 bits"),
])
def test_a_malformed_line_is_named(text, line, what):
    from kmergutsjava_amd import make_table as M
    with pytest.raises(M.SignatureFormatError) as ei:
        M.parse_signatures(text.encode())
    assert ei.value.line == line
    assert ("line %d:" % line) in str(ei.value) and what in str(ei.value)


def test_default_prime_agrees_with_trial_division():
    from kmergutsjava_amd import make_table as M
    N = 10 ** 5
    sieve = np.ones(N + 1, dtype=bool)
    sieve[:2] = False
    for p in range(2, int(N ** 0.5) + 1):
        if sieve[p]:
            sieve[p * p::p] = False
    assert [n for n in range(N + 1) if M.is_prime(n)] == np.flatnonzero(sieve).tolist()
    nxt = np.empty(N + 1, dtype=np.int64)
    p = 100003                                      # the smallest prime above 10^5
    for n in range(N, -1, -1):
        if sieve[n]:
            p = n
        nxt[n] = p
    assert all(M.next_prime(n) == max(int(nxt[n]), 2) for n in range(0, N + 1, 7))
    assert M.default_num_sigs(0) == 2 and M.default_num_sigs(500000) == 1000003


def test_default_prime_at_64_bit_values():
    from kmergutsjava_amd import make_table as M

    def trial(n):
        if n < 2:
            return False
        f = 2
        while f * f <= n:
            if n % f == 0:
                return False
            f += 1
        return True
    # known primes / composites, including strong pseudoprimes to several small bases
    assert M.is_prime(2 ** 61 - 1) and M.is_prime(2 ** 64 - 59) and M.is_prime(18446744073709551557)
    assert not M.is_prime(2 ** 64 - 1) and not M.is_prime(3215031751) and not M.is_prime(3825123056546413051)
    assert not M.is_prime((2 ** 31 - 1) * (2 ** 31 - 1)) and not M.is_prime(4294967297)
    assert M.next_prime(2 ** 64 - 100) == 2 ** 64 - 95 and M.next_prime(2 ** 64 - 82) == 2 ** 64 - 59
    for n in (2 ** 32 - 10, 10 ** 12 + 30, 1_400_303_150):          # sqrt within reach of trial division
        assert M.next_prime(n) == next(m for m in range(n, n + 10 ** 4) if trial(m))
