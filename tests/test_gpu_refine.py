"""The 32-bit build's refinement stages at their group and tile edges (cases and model: tests/refine_cases.py): every build
is compared whole with the oracle, verified on the device, AND its BuildStats counts are compared with the model, exactly --
a stage that drops or mis-plans a group at an edge still yields the right array, because a later stage repairs it, but not
the right counts.

Texts of 27 symbols with SA_HIP_INITIAL_CHARS=12 (12 symbols of 5 bits: the key length is known; the two cases over 4 and 256
symbols ask for 21 and 7 symbols and read initial_chars back like the others; a key of more than 56 bits takes the
12-byte-record sort, so an int64 copy comes from the widening pass at the end -- the patched copy of the narrow plan needs a
key of <= 40 bits and has its own test in test_gpu_build.py).

Counts the model vouches for: tiny_resolved, finisher_runs / finisher_records / finisher_resolved, and rounds, chunk_rounds,
active_total as long as the build stays in chunk rounds (simulate's `exact`); beyond that they are lower bounds and
doubling_rounds > 0.  radix_records / radix_passes count every pass of the global sort, the initial sort's included: a round
adds (records of the groups its plan left out) x (passes), so radix_records == n x initial passes + that sum.
period_resolved is the model's (refine_cases.period_attempt): 0 in the first three families, exact in the fourth.
loc_big_copy_kernel cuts every left-out group into 16 slices whatever its size, so the round sort's big group of 20 000 records
takes the same path as one of 10^5 would."""
import numpy as np
import pytest

import refine_cases as rc

pytestmark = pytest.mark.gpu

SWITCHES = ("SA_HIP_TINY", "SA_HIP_PERIOD_FINISH", "SA_HIP_GROUP_FINISH", "SA_HIP_FIN_LEFT_FAST", "SA_HIP_LOCAL_ROUNDS",
            "SA_HIP_INITIAL_CHARS")
_memo = {}


@pytest.fixture(autouse=True)
def _drop_memo():
    """texts, groups and expected arrays are shared by the variants inside one test function only"""
    yield
    _memo.clear()


def prepared(oracle, family, name, case, cap, k=None):
    """text, expected array, groups of a case: computed once per test function"""
    key = (family, name, k)
    if key not in _memo:
        t = rc.make_periodic(case) if isinstance(case, rc.PCase) else rc.make(case)
        b = max(1, int(np.unique(t).size).bit_length())
        sa = oracle.sais(t).astype(np.int64)
        g = rc.groups_after_keys(t, sa, k or 64 // b, cap)
        L = getattr(case, "L", 0)
        want = oracle.truncated_sa(t, L).astype(np.int64) if L else sa
        _memo[key] = (t, b, g, want, sa)
    return _memo[key]


def build(gpu, monkeypatch, t, L, env, wide=False):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with gpu.DeviceIndex(t.size, 0) as idx:
        idx.build(t, L)
        if wide:
            import torch
            out = torch.full((t.size + 2,), -7, dtype=torch.int64, device="cuda:0")
            torch.cuda.synchronize()
            idx.build_device64(idx.text_dev, t.size, out.data_ptr(), L)
            idx.sync()
        st = idx.build_stats()
        assert idx.verify() == 0, st
        sa = idx.sa_u32().astype(np.int64)
        if wide:
            got = out.cpu().numpy()
            assert np.array_equal(got[:t.size], sa) and (got[t.size:] == -7).all(), st
    return sa, st


def check(st, m, g, n, b, k, tag):
    print(tag, {x: st[x] for x in ("tiny_resolved", "finisher_runs", "finisher_records", "finisher_resolved", "period_resolved", "rounds",
                                   "chunk_rounds", "doubling_rounds", "active_total", "radix_records", "radix_passes")},
          "model", {x: v for x, v in m.items() if x not in ("plans", "round_sizes")})
    assert st["initial_chars"] == k and st["bits_per_symbol"] == b and st["narrow48"] == 0, (tag, st)
    for x in ("tiny_resolved", "finisher_runs", "finisher_records", "finisher_resolved"):
        assert st[x] == m[x], (tag, x, st[x], m[x])
    assert st["period_resolved"] == m["period_resolved"], (tag, st["period_resolved"], m["period_resolved"])
    initial_passes = -(-(b * k) // 8)
    if m["exact"]:
        for x in ("rounds", "chunk_rounds", "active_total"):
            assert st[x] == m[x], (tag, x, st[x], m[x])
        assert st["doubling_rounds"] == 0, (tag, st)
        if k == 64 // b:   # (the 12-byte-record sort; a narrow-record sort counts its passes differently)
            assert st["radix_records"] == n * initial_passes + m["big_passes_records"], (tag, st["radix_records"], n, m["big_passes_records"])
    else:
        # the model stopped before a doubling round of `handover` records: that round is counted too
        assert st["doubling_rounds"] > 0 and st["chunk_rounds"] == m["chunk_rounds"], (tag, st)
        assert st["rounds"] > m["rounds"] and st["active_total"] >= m["active_total"] + m["handover"] > m["active_total"], (tag, st, m["handover"])


def run(gpu, oracle, monkeypatch, family, name, case, env, sim, cap=256, wide=False, tag="", k=None):
    t, b, g, want, full = prepared(oracle, family, name, case, cap, k)
    k = k or 64 // b
    e = dict(env)
    e["SA_HIP_INITIAL_CHARS"] = str(k)   # 12 at 27 symbols, 21 at 4, 7 at 256: as many symbols as 64 bits hold; asserted in check()
    L = getattr(case, "L", 0)
    sa, st = build(gpu, monkeypatch, t, L, e, wide)
    assert np.array_equal(sa, want), (family, name, tag, st, int(np.flatnonzero(sa != want)[0]))
    m = rc.simulate(g, int(t.size), k, b, L=L, t=t, sa=full, **sim)
    check(st, m, g, int(t.size), b, k, "%s/%s%s" % (family, name, tag))
    return sa, st, m, g


CAPS = {"long_lcp": 4400, "below_a_quarter": 1000, "above_a_quarter": 1000}


@pytest.mark.parametrize("name", list(rc.tiny_cases()))
def test_tiny_finisher(gpu, oracle, monkeypatch, name):
    """default settings: groups of 2..8 that come apart within 64 bytes are written by the tiny pass, the rest reaches the group
    finisher (and, for the pairs that share 64 and 65 bytes, the rounds) exactly as modelled"""
    case = rc.tiny_cases()[name]
    sa, st, m, g = run(gpu, oracle, monkeypatch, "tiny", name, case, {}, {}, wide=name in ("sizes_2_9", "ends_at_text_end"))
    if name == "sparse_16M_gt_n":
        assert st["tiny_resolved"] == 0 and st["finisher_resolved"] == g.M
    elif name != "lcp_63_64_65":
        assert st["tiny_resolved"] > 0 and st["rounds"] == 0


@pytest.mark.parametrize("name", list(rc.finisher_cases()))
def test_group_finisher(gpu, oracle, monkeypatch, name):
    """SA_HIP_TINY=0, SA_HIP_PERIOD_FINISH=0; the default kernel and the done-flag path give the same numbers"""
    case = rc.finisher_cases()[name]
    base = {"SA_HIP_TINY": "0", "SA_HIP_PERIOD_FINISH": "0"}
    sim = dict(tiny=False, period_finish=False)
    first = None
    for tag, extra in (("", {}), ("+flags", {"SA_HIP_FIN_LEFT_FAST": "0"})):
        sa, st, m, g = run(gpu, oracle, monkeypatch, "fin", name, case, dict(base, **extra), sim, cap=CAPS.get(name, 256),
                           wide=(tag == "" and name in ("tile_cap_plus_1", "long_lcp")), tag=tag)
        if first is None:
            first = sa
        assert np.array_equal(sa, first)


@pytest.mark.parametrize("name", list(rc.round_sort_cases()))
def test_round_sort_in_lds(gpu, oracle, monkeypatch, name):
    """SA_HIP_GROUP_FINISH=0, SA_HIP_TINY=0, SA_HIP_PERIOD_FINISH=0: every tied record through the rounds.  The record form of
    loc_sort_kernel is the model's loc_sort_packed (Builder::round_sort's rule restated): a full build's first chunk round at
    b = 5 or 9 appends (64 - gb) / b symbols, more than 40 key bits, so it takes the unpacked form; the build truncated at
    L = 20 appends 8 symbols = 40 bits and takes the packed one.  With SA_HIP_LOCAL_ROUNDS=0 every record goes through the
    global sort and the array is the same."""
    case = rc.round_sort_cases()[name]
    base = {"SA_HIP_TINY": "0", "SA_HIP_PERIOD_FINISH": "0", "SA_HIP_GROUP_FINISH": "0"}
    sim = dict(tiny=False, period_finish=False, group_finish=False)
    sa, st, m, g = run(gpu, oracle, monkeypatch, "loc", name, case, base, sim, wide=name == "tile_cap_plus_1")
    assert m["packed"][0] == (name == "packed_L20")
    sa0, st0, m0, _ = run(gpu, oracle, monkeypatch, "loc", name, case, dict(base, SA_HIP_LOCAL_ROUNDS="0"), dict(sim, local_rounds=False),
                          tag="+global")
    assert np.array_equal(sa, sa0)
    assert st["active_total"] == st0["active_total"] and st["rounds"] == st0["rounds"]


@pytest.mark.parametrize("name", list(rc.period_cases()))
def test_period_finisher(gpu, oracle, monkeypatch, name):
    """default settings, full arrays: the groups of a periodic run are left by the tiny pass (a pair of each shares 64 symbols
    or more), the finisher gives up on them, and the shortcut is tried on M >= 64 records; period_resolved is the model's.
    E == p0 + (m - 2) d itself cannot occur (the last two members share the key, so the run reaches K symbols further or ends
    before them): E_one_less ends it one symbol before, E_first_reachable K symbols after."""
    case = rc.period_cases()[name]
    sa, st, m, g = run(gpu, oracle, monkeypatch, "per", name, case, {}, {}, cap=512, wide=name in ("ends_lt_gt_eot", "E_one_less"))
    if name == "M63":
        assert st["period_resolved"] == 0 and m["handover"] == 63
    else:
        assert st["period_resolved"] > 0


@pytest.mark.parametrize("name", list(rc.narrow_cases()))
def test_int64_copy_patched_after_refinement(gpu, oracle, monkeypatch, name):
    """sa_hip_index_build_device64 on the narrow-record plan (SA_HIP_INITIAL_CHARS=8: a 40-bit key; the plan needs 2^22
    symbols): the sort's last pass writes the int64 copy (widen_fused) and refinement patches it.  all_tiny: the tiny pass
    resolves every tied record and writes both widths itself (patched_by_tiny: tiny_resolved == M, nothing else runs);
    with_rest: groups of 9 go on to the group finisher, so widen_patch_kernel rewrites the slots of the first active list."""
    case = rc.narrow_cases()[name]
    sa, st, m, g = run(gpu, oracle, monkeypatch, "narrow", name, case, {}, {}, wide=True, k=8)
    assert st["widen_fused"] == 1 and st["initial_chars"] == 8, st
    if name == "all_tiny":
        assert st["tiny_resolved"] == g.M and st["finisher_runs"] == 0 and st["rounds"] == 0, st
    else:
        assert 0 < st["tiny_resolved"] < g.M and st["finisher_resolved"] == g.M - st["tiny_resolved"], st
