"""The two device arrays every token search starts from -- dir, the first-symbol directory, and K, the key array
(csrc/token_query.hpp: tq_range searches only [dir[v - min], dir[v - min + 1]) and reads K instead of the text) -- read back through
sa_hip_token_index_get_dir_range / _get_key_range and compared with the NumPy models of tests/token_struct_cases.py, every entry,
exactly; then the same entries through the search (one length-1 pattern per value of [min - 1, max + 1], built on the device),
the two one-loop bounds (tq_key_bounds, tq_text_bounds) on every window size 1 .. 65 and around 128 and 256 with every short
pattern, and the key array as tq_next_symbol reads it.  A wrong entry of either array does not fault: it narrows or shifts the
search for the patterns of one symbol or one key group, and the other tests ask a few thousand sampled patterns per text.

Handles are made with load_device from the model suffix array -- a failure here is not a failure of the build --; one text per
family also goes through TokenIndex.build and must hold the same bytes."""
import numpy as np
import pytest

import token_cases as tc
import token_next_cases as nc
import token_struct_cases as sc

pytestmark = pytest.mark.gpu

GUARD32, GUARD64 = 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _load(gpu, t, sa):
    import torch
    t_d, sa_d = _dev(t), _dev(np.asarray(sa, np.int32))
    torch.cuda.synchronize()
    return gpu.TokenIndex.load_device(t_d.data_ptr() if t.size else None, sa_d.data_ptr() if t.size else None, t.size)   # (copied into the handle)


def _same_across_plans(seen, key, plan, data, errors):
    """seen: a dict of the one test function that runs all its plans -- the comparison cannot be deselected"""
    first = seen.setdefault(key, (plan, data))
    if first[1] != data:
        errors.append("%s: plan %s does not answer byte for byte what plan %s answered" % (key, plan, first[0]))


def _refused(lib, call, word):
    return call() == -1 and word in lib.sa_hip_last_error()


def _singles(ti, v0, q):
    """the device form over the patterns [v0], [v0 + 1], ..., built on the device -> uint32[q, 2]"""
    import torch
    pat = torch.arange(v0, v0 + q, dtype=torch.int64, device="cuda:0").to(torch.int32)
    off = torch.arange(0, q + 1, dtype=torch.int64, device="cuda:0")
    out = torch.full((q, 2), -1, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    ti.query_batch_device(pat.data_ptr(), off.data_ptr(), q, out.data_ptr())
    ti.sync()
    return out.cpu().numpy().view(np.uint32)


# ---- read-backs ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("plan", list(tc.PLANS))
def test_directory_and_keys_entry_by_entry(gpu, monkeypatch, plan):
    """dir under default and no_keys, K under default and no_dir, every entry against the model; info(); and the refusal where the
    plan or the range leaves no structure"""
    tc.set_plan(monkeypatch, plan)
    lib = gpu.lib()
    errors = []
    one32, one64 = np.zeros(1, np.uint32), np.zeros(1, np.uint64)
    for name in sc.DIR_TEXTS:
        t, sa = sc.text(name), sc.sa_of(name)
        want = sc.info_expected(name, plan)
        with _load(gpu, t, sa) as ti:
            info = ti.info()
            got = {k: info[k] for k in want}
            if got != want:
                errors.append("%s/%s: info %s, model %s" % (name, plan, got, want))
                continue
            if want["dir_entries"]:
                why = sc.mismatch("dir", ti.dir_range(0, want["dir_entries"]), sc.dir_of(name), t, sa)
                if why:
                    errors.append("%s/%s: %s" % (name, plan, why))
            elif not _refused(lib, lambda: lib.sa_hip_token_index_get_dir_range(ti._h, 0, 1, one32.ctypes.data), b"no directory"):
                errors.append("%s/%s: dir_range is not refused: %r" % (name, plan, lib.sa_hip_last_error()))
            if want["key_bytes"]:
                why = sc.mismatch("K", ti.key_range(0, t.size), sc.keys_of(name), t, sa)
                if why:
                    errors.append("%s/%s: %s" % (name, plan, why))
            elif not _refused(lib, lambda: lib.sa_hip_token_index_get_key_range(ti._h, 0, 1, one64.ctypes.data), b"no key array"):
                errors.append("%s/%s: key_range is not refused: %r" % (name, plan, lib.sa_hip_last_error()))
    assert not errors, "%d mismatches:\n%s" % (len(errors), "\n".join(errors[:20]))


def test_read_backs_refuse_and_take_parts(gpu, monkeypatch):
    """n == 0 leaves no structure; first + count one past the end is refused; a part of the range lands between two guard words"""
    tc.set_plan(monkeypatch, "default")
    lib = gpu.lib()
    buf32, buf64 = np.full(8, GUARD32, np.uint32), np.full(8, GUARD64, np.uint64)
    with gpu.TokenIndex.load_device(None, None, 0) as ti:
        assert _refused(lib, lambda: lib.sa_hip_token_index_get_dir_range(ti._h, 0, 0, buf32.ctypes.data), b"no directory")
        assert _refused(lib, lambda: lib.sa_hip_token_index_get_key_range(ti._h, 0, 0, buf64.ctypes.data), b"no key array")
        with pytest.raises(gpu.SaHipError):
            ti.dir_range(0, 0)
        with pytest.raises(gpu.SaHipError):
            ti.key_range(0, 1)
    for name in ("tile_8193", "top_of_range", "equal_1"):
        t = sc.BOUNDS_TEXTS[name] if name in sc.BOUNDS_TEXTS else sc.text(name)
        sa = sc.bounds_expected(name)[1] if name in sc.BOUNDS_TEXTS else sc.sa_of(name)
        d, k = sc.directory(t), sc.keys(t, sa)
        n, L = t.size, d.size
        with _load(gpu, t, sa) as ti:
            for first, count in ((0, L + 1), (L, 1), (1, L), (L + 1, 0), (2 ** 63, 2 ** 63), (2 ** 64 - 1, 2)):
                assert _refused(lib, lambda: lib.sa_hip_token_index_get_dir_range(ti._h, first, count, buf32.ctypes.data), b"beyond"), (name, first, count)
            for first, count in ((0, n + 1), (n, 1), (1, n), (n + 1, 0), (2 ** 63, 2 ** 63), (2 ** 64 - 1, 2)):
                assert _refused(lib, lambda: lib.sa_hip_token_index_get_key_range(ti._h, first, count, buf64.ctypes.data), b"beyond"), (name, first, count)
            assert lib.sa_hip_token_index_get_dir_range(ti._h, 0, 1, None) == -1 and lib.sa_hip_token_index_get_key_range(ti._h, 0, 1, None) == -1
            assert (buf32 == GUARD32).all() and (buf64 == GUARD64).all()                 # a refused call writes nothing
            assert ti.dir_range(L, 0).size == 0 and ti.key_range(n, 0).size == 0           # an empty range at the end
            for first, count in ((0, 1), (L - 1, 1), (max(L - 6, 0), min(6, L)), (L // 2, min(5, L - L // 2))):
                b = np.full(count + 2, GUARD32, np.uint32)
                assert lib.sa_hip_token_index_get_dir_range(ti._h, first, count, b[1:].ctypes.data) == 0, (name, first, count)
                assert b[0] == GUARD32 and b[-1] == GUARD32 and np.array_equal(b[1:-1], d[first:first + count]), (name, first, count)
            for first, count in ((0, 1), (n - 1, 1), (max(n - 6, 0), min(6, n)), (n // 2, min(5, n - n // 2))):
                b = np.full(count + 2, GUARD64, np.uint64)
                assert lib.sa_hip_token_index_get_key_range(ti._h, first, count, b[1:].ctypes.data) == 0, (name, first, count)
                assert b[0] == GUARD64 and b[-1] == GUARD64 and np.array_equal(b[1:-1], k[first:first + count]), (name, first, count)
            assert np.array_equal(ti.dir_range(0, L), d) and np.array_equal(ti.key_range(0, n), k)


def test_build_holds_the_bytes_of_load(gpu, monkeypatch):
    """one text per family through TokenIndex.build: the suffix array, both structures and the answers, byte for byte"""
    tc.set_plan(monkeypatch, "default")
    for name in sc.FAMILIES + ("equal_65", "period2_64", "random_63", "equal_but_last_257"):
        small = name in sc.BOUNDS_TEXTS
        t = sc.BOUNDS_TEXTS[name] if small else sc.text(name)
        sa = sc.bounds_expected(name)[1] if small else sc.sa_of(name)
        with _load(gpu, t, sa) as a, gpu.TokenIndex.build(t) as b:
            ia, ib = a.info(), b.info()
            assert {k: ia[k] for k in ("n", "min_symbol", "max_symbol", "dir_entries", "key_bytes", "last_rank")} == \
                   {k: ib[k] for k in ("n", "min_symbol", "max_symbol", "dir_entries", "key_bytes", "last_rank")}, name
            assert b.sa_range(0, t.size).tobytes() == np.asarray(sa, np.int32).tobytes(), name
            assert b.key_range(0, t.size).tobytes() == a.key_range(0, t.size).tobytes(), name
            assert b.dir_range(0, ia["dir_entries"]).tobytes() == a.dir_range(0, ia["dir_entries"]).tobytes(), name
            if small:
                pats = sc.packed_patterns(name)
                assert b.query_batch(pats).tobytes() == a.query_batch(pats).tobytes(), name
            else:
                v0, q, _, _ = sc.singles_expected(name)
                assert _singles(b, v0, q).tobytes() == _singles(a, v0, q).tobytes(), name


# ---- the same entries through the search -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sc.DIR_TEXTS)
def test_every_symbol_of_the_range_through_the_search(gpu, monkeypatch, name):
    """[v] for every v of [min - 1, max + 1] in one device-form batch: first is searchsorted over the sorted text, count is
    bincount, the absent symbols included; the texts of a small range under all four plans, byte for byte the same"""
    t, sa = sc.text(name), sc.sa_of(name)
    v0, q, first, count = sc.singles_expected(name)
    errors, seen = [], {}
    for plan in (list(tc.PLANS) if sc.range_of(name) <= sc.SMALL_RANGE else ["default"]):
        tc.set_plan(monkeypatch, plan)
        with _load(gpu, t, sa) as ti:
            got = _singles(ti, v0, q)
            assert ti.info()["q"] == q
        bad = np.flatnonzero((got[:, 0] != first) | (got[:, 1] != count))
        if bad.size:
            errors.append("%s/%s: %d of %d patterns differ\n" % (name, plan, bad.size, q) + "\n".join(
                "  [%d]: got (%d, %d), model (%d, %d) -- %s" % (v0 + i, got[i, 0], got[i, 1], first[i], count[i],
                                                               sc.describe("dir", t, sa, max(int(i) - 1, 0)) if sc.has_directory(t) else "no directory")
                for i in bad[:5]))
        _same_across_plans(seen, name, plan, got.tobytes(), errors)
    assert not errors, "\n".join(errors)


# ---- bounds ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", ["equal", "period2", "random", "equal_but_last"])
def test_bounds_at_every_window_size(gpu, monkeypatch, family):
    """every bounds text under all four plans, its whole pattern set in one batch: both fields against model (a), the counts against
    model (b), the four answers byte for byte the same"""
    errors, seen = [], {}
    for plan in tc.PLANS:
        tc.set_plan(monkeypatch, plan)                                         # (read when a handle is made)
        for name in sc.BOUNDS_TEXTS:
            if name.rsplit("_", 1)[0] != family:
                continue
            t, sa, pats, first, count, count_b = sc.bounds_expected(name)
            with _load(gpu, t, sa) as ti:
                got = ti.query_batch(sc.packed_patterns(name))
            bad = np.flatnonzero((got["first"] != first) | (got["second"] != count) | (got["second"] != count_b))
            if bad.size:
                errors.append("%s/%s: %d of %d patterns differ: %s" % (name, plan, bad.size, len(pats), [
                    (pats[i][:8], len(pats[i]), (int(got["first"][i]), int(got["second"][i])), (int(first[i]), int(count[i]), int(count_b[i]))) for i in bad[:5]]))
            _same_across_plans(seen, name, plan, got.tobytes(), errors)
    assert len(seen) == {"equal": 71, "period2": 65, "random": 65, "equal_but_last": 6}[family]
    assert not errors, "%d mismatches:\n%s" % (len(errors), "\n".join(errors[:20]))


@pytest.mark.parametrize("family", ["equal", "period2", "random", "equal_but_last"])
def test_longest_suffix_spans_on_the_bounds_texts(gpu, monkeypatch, family):
    """spans_batch in mode 1 under every configuration, the contexts the short patterns and the whole text, against
    token_next_cases.spans_a over the model suffix array"""
    tc.set_plan(monkeypatch, "default")
    errors = []
    names = [n for n in sc.BOUNDS_TEXTS if n.rsplit("_", 1)[0] == family]
    assert len(names) == {"equal": 71, "period2": 65, "random": 65, "equal_but_last": 6}[family]
    for name in names:
        t, sa = sc.bounds_expected(name)[:2]
        ctx = sc.span_contexts(t)
        packed = tc.pack(ctx)
        tl, sl = [int(v) for v in t], [int(v) for v in sa]
        with _load(gpu, t, sa) as ti:
            for cfg in nc.CONFIGS:
                if cfg[0] != 1:
                    continue
                want = nc.spans_a(tl, sl, ctx, *cfg)
                got = ti.spans_batch(packed, *cfg)
                got = np.stack([got[f] for f in ("first", "count", "length", "ended")], axis=1)
                bad = np.flatnonzero((got != want).any(axis=1))
                if bad.size:
                    errors.append("%s %s: %d of %d contexts differ: %s" % (name, cfg, bad.size, len(ctx), [
                        (ctx[i][:8], len(ctx[i]), got[i].tolist(), want[i].tolist()) for i in bad[:5]]))
    assert not errors, "%d mismatches:\n%s" % (len(errors), "\n".join(errors[:20]))


# ---- feeding the walks -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sc.WALK_TEXTS)
def test_keys_feed_the_next_symbol_short_cut(gpu, monkeypatch, name):
    """next_of_spans over (r, 1, 0) and (r, 1, 1): tq_next_symbol reads the high and the low field of K[r]; without the key array it
    reads T[SA[r] + length], and both answer the fields of the model minus 1"""
    t, sa, k = sc.text(name), sc.sa_of(name), sc.keys_of(name)
    n = t.size
    r = np.linspace(0, n - 1, sc.WALK_RANKS).astype(np.int64)
    r[sc.WALK_RANKS // 2] = sc.info_expected(name, "default")["last_rank"]           # the suffix without a next symbol
    hi = (k[r] >> np.uint64(32)).astype(np.int64) - 1
    lo = (k[r] & np.uint64(0xFFFFFFFF)).astype(np.int64) - 1
    assert np.array_equal(hi, t[sa[r]]) and int((lo < 0).sum()) == 1
    errors, seen = [], {}
    for plan in ("default", "no_keys"):
        tc.set_plan(monkeypatch, plan)
        with _load(gpu, t, sa) as ti:
            for length, want in ((0, hi), (1, lo)):
                spans = np.zeros(r.size, gpu.SPAN_DTYPE)
                spans["first"], spans["count"], spans["length"] = r, 1, length
                spans["ended"] = (sa[r].astype(np.int64) + length == n)
                got = ti.next_of_spans(spans, cap=1, fill=-7)
                has = want >= 0
                sym, cnt, wr = got["symbols"][:, 0], got["counts"][:, 0], got["heads"]["written"]
                bad = np.flatnonzero((wr != has) | (sym != np.where(has, want, -7)) | (cnt != np.where(has, 1, (-7) & 0xFFFFFFFF)) |
                                     (got["heads"]["total"] != has))
                if bad.size:
                    errors.append("%s/%s length %d: %d of %d ranks differ: %s" % (name, plan, length, bad.size, r.size, [
                        (int(sym[i]), int(cnt[i]), int(wr[i]), int(want[i]), sc.describe("K", t, sa, r[i])) for i in bad[:5]]))
                _same_across_plans(seen, length, plan, sym.tobytes() + cnt.tobytes() + got["heads"].tobytes(), errors)
    assert not errors, "\n".join(errors)
