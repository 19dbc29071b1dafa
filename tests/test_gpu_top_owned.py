"""The owned-run body of the top-digit pass's claim form (csrc/radix_narrow.hpp: text_top_owned_tile) at its tile, lane, window
and alphabet edges.  Thread tid of a tile of 8192 positions owns positions 16 tid .. 16 tid + 15, loads the 24 text bytes that
end with the last character of its 16th key, rolls the codes through one window and ranks by a returning LDS atomic on 2048
fine bins; the tile takes the body without checks when 8192 + 24 bytes lie below n.

Every case is built three times -- the owned-run body (default), SA_HIP_TOP_OWNED=0 (the previous claim body) and
SA_HIP_TOP_CLAIMS=0 (the stable form) -- and the three must agree with each other and with the oracle: verify(), the suffix
array, the int64 copy with the guard words behind it, the query ranges (hits, misses, what starts and what ends the text) and
the plan's statistics.

Lengths: the narrow-record sort, and with it this pass, only runs from 2^22 positions on (narrow_sort_applies), and 2^22 is a
multiple of the tile.  The lengths are therefore 2^22 + 8192 t + r, t in {1, 2}: every r in {0, 1, 15, 16, 17, 63, 64, 65, 8191}
(a last tile of 1, 15, 16, 17 positions, a last lane whose window crosses n, both sides of the checked / unchecked decision),
r in {23, 24, 25} around the 24 bytes that decision looks ahead, and five tiles plus one position.  Alphabets and keys: 5 bits
x 8 (D1's), x 7 (the lane at the start of the text looks before it), 8 bits x 5, 3 bits x 9, 3 bits x 13 (longer than the window
covers: the previous claim body), byte 0 as a symbol that also ends the text, one character repeated over the first 40
positions (two lanes, 32 records, one fine bin)."""
import numpy as np
import pytest

import cases
from refine_cases import D1_SYMBOLS

pytestmark = pytest.mark.gpu

BASE = 1 << 22
TILE = 8192
SWITCHES = ("SA_HIP_SPLIT", "SA_HIP_SPLIT_CAP", "SA_HIP_INITIAL_CHARS", "SA_HIP_TOP_OWNED", "SA_HIP_TOP_CLAIMS")
FORMS = (("owned", {}), ("claim", {"SA_HIP_TOP_OWNED": "0"}), ("stable", {"SA_HIP_TOP_CLAIMS": "0"}))
STATS = ("split_plan", "radix_passes", "lite_flags", "active_total")
_pool = {}


def _random(name, symbols, n, seed):
    """the first n symbols of one random text per alphabet (drawn once at the largest length)"""
    if name not in _pool:
        _pool[name] = np.asarray(symbols, np.uint8)[np.random.default_rng(seed).integers(0, len(symbols), BASE + 6 * TILE)]
    return _pool[name][:n].copy()


def d1(n):
    return _random("d1", D1_SYMBOLS, n, 31)


def byte0(n):
    """byte 0 is the smallest of 27 symbols (code 1, not the padding's code 0) and the text's last three symbols"""
    t = _random("byte0", [0] + sorted(D1_SYMBOLS.tolist())[1:], n, 32)
    t[-3:] = 0
    return t


def repeated(n):
    t = d1(n)
    t[:40] = t[100]
    return t


def wide(n):
    return _random("wide", np.arange(40, 240), n, 33)


def dna(n):
    return _random("dna", np.frombuffer(b"acgt", np.uint8), n, 34)


RS = (0, 1, 15, 16, 17, 63, 64, 65, 8191)
CASES = [("d1_t%d_r%d" % (t, r), d1, BASE + TILE * t + r, 8) for t in (1, 2) for r in RS]
CASES += [("d1_t1_r%d" % r, d1, BASE + TILE + r, 8) for r in (23, 24, 25)]
CASES += [
    ("d1_t5_r1", d1, BASE + 5 * TILE + 1, 8),
    ("d1_k7", d1, BASE + TILE + 17, 7),
    ("b8_k5", wide, BASE + TILE + 17, 5),
    ("b3_k9", dna, BASE + TILE + 17, 9),
    ("b3_k13_beyond_window", dna, BASE + TILE + 17, 13),
    ("byte0", byte0, BASE + TILE + 15, 8),
    ("repeated_start", repeated, BASE + TILE + 65, 8),
]


def patterns(t, k0):
    rng = np.random.default_rng(7)
    pats = cases.query_patterns(t, 200, rng, maxlen=k0 + 6)
    pats += [bytes(t[:j]) for j in range(1, k0 + 4)]                      # what starts the text
    pats += [bytes(t[-j:]) for j in range(1, k0 + 4)]                     # what ends it
    pats += [bytes(t[-j:]) + bytes(t[:1]) for j in range(1, k0 + 2)]      # ... and one symbol more: beyond the end
    absent = int(np.flatnonzero(np.bincount(t, minlength=256) == 0)[0])
    pats += [bytes([absent]), bytes(t[5:5 + k0 - 1]) + bytes([absent]), bytes(t[-3:]) + bytes([absent])]
    return pats


@pytest.mark.parametrize("name,make,n,k0", CASES, ids=[c[0] for c in CASES])
def test_three_forms_agree_with_the_oracle(gpu, oracle, monkeypatch, name, make, n, k0):
    import torch
    t = make(n)
    assert t.size == n
    want = oracle.sais(t).astype(np.int64)
    pats = patterns(t, k0)
    want_q = oracle.query_batch(t, want.astype(np.uint32), 0xFFFFFFFF, pats)
    stats = {}
    errors = []
    for tag, fenv in FORMS:
        for k in SWITCHES:
            monkeypatch.delenv(k, raising=False)
        monkeypatch.setenv("SA_HIP_SPLIT", "1")
        monkeypatch.setenv("SA_HIP_INITIAL_CHARS", str(k0))
        for k, v in fenv.items():
            monkeypatch.setenv(k, v)
        with gpu.DeviceIndex(n, 0) as idx:
            idx.build(t)
            bad = idx.verify()
            sa = idx.sa_u32().astype(np.int64)
            got_q = idx.query_batch(pats)
            out = torch.full((n + 2,), -7, dtype=torch.int64, device="cuda:0")
            torch.cuda.synchronize()
            idx.build_device64(idx.text_dev, n, out.data_ptr(), 0)
            idx.sync()
            st = idx.build_stats()
            wide_sa = out.cpu().numpy()
        stats[tag] = {x: st[x] for x in STATS}
        print(name, tag, stats[tag], {x: st[x] for x in ("initial_chars", "bits_per_symbol", "text_top_pass", "split_max")})
        if bad != 0:
            errors.append("%s: verify() = %d" % (tag, bad))
        if not np.array_equal(sa, want):
            errors.append("%s: array differs from the oracle, first at slot %d" % (tag, int(np.flatnonzero(sa != want)[0])))
        if not np.array_equal(wide_sa[:n], want):
            errors.append("%s: int64 copy differs from the oracle, first at slot %d" % (tag, int(np.flatnonzero(wide_sa[:n] != want)[0])))
        if not (wide_sa[n:] == -7).all():
            errors.append("%s: guard words behind the int64 copy written: %s" % (tag, wide_sa[n:].tolist()))
        if not np.array_equal(got_q, want_q):
            i = int(np.flatnonzero(got_q != want_q)[0])
            errors.append("%s: query %r: %s, oracle %s" % (tag, pats[i], got_q[i], want_q[i]))
        if st["initial_chars"] != k0 or st["text_top_pass"] != 1 or st["split_plan"] == 0 or st["radix_passes"] != 3:
            errors.append("%s: the plan was not taken as the case means it: %s" % (tag, st))
    for tag in ("claim", "stable"):
        if stats[tag] != stats["owned"]:
            errors.append("%s: statistics %s, owned-run body %s" % (tag, stats[tag], stats["owned"]))
    assert not errors, "\n".join(errors)
