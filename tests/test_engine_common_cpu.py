"""What the engines share by rule (``models/common.py``): the per-stream scratch pool, and the two rules of the statistics
hand-off against literal restatements of the rules each engine carried before they were merged.  No GPU, nothing launched."""
import itertools
import types

import pytest
import torch

from vdpp_amd.models import common


# ------------------------------------------------------------------------------------------------ StreamScratch
@pytest.fixture
def streams(monkeypatch):
    """``current[0]`` is the raw handle ``torch.cuda.current_stream`` reports."""
    current = [0x1000]
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a, **k: types.SimpleNamespace(cuda_stream=current[0]))
    return current


def span(t):
    return t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()


def test_stream_scratch_holds_one_buffer_per_stream_and_name(streams):
    pool = common.StreamScratch("cpu")
    got = {}
    for handle in (0x1000, 0x2000):
        streams[0] = handle
        for name in ("gn", "splitk", "fp8", "long"):
            got[handle, name] = pool.get(name, 4096)
    assert all(t.dtype == torch.uint8 and t.numel() == 4096 for t in got.values())
    assert len({id(t) for t in got.values()}) == 8
    # two names never overlap in memory ("gn" and "splitk" are live together for the length of a forward), nor two streams
    for a, b in itertools.combinations(got.values(), 2):
        (a0, a1), (b0, b1) = span(a), span(b)
        assert a1 <= b0 or b1 <= a0
    # an equal or a smaller request returns the same object, on either stream
    for (handle, name), t in got.items():
        streams[0] = handle
        assert pool.get(name, 4096) is t and pool.get(name, 1) is t and pool.get(name, 0) is t


def test_stream_scratch_grows_one_entry_only(streams):
    pool = common.StreamScratch("cpu")
    gn, sk = pool.get("gn", 1000), pool.get("splitk", 1000)
    streams[0] = 0x2000
    other = pool.get("gn", 1000)
    streams[0] = 0x1000
    big = pool.get("gn", 1001)
    assert big is not gn and big.numel() == 1001
    assert pool.get("gn", 1000) is big and pool.get("splitk", 1000) is sk
    streams[0] = 0x2000
    assert pool.get("gn", 1000) is other


def test_stream_scratch_floor_and_clear(streams):
    pool = common.StreamScratch("cpu")
    a = pool.get("gn", 100, floor=1 << 20)
    assert a.numel() == 1 << 20
    assert pool.get("gn", 1 << 20, floor=1 << 20) is a and pool.get("gn", 5000) is a
    b = pool.get("gn", (1 << 20) + 1, floor=1 << 20)            # beyond the floor: the request itself
    assert b is not a and b.numel() == (1 << 20) + 1
    assert pool.get("long", 64).numel() == 64                   # no floor unless asked for
    pool.clear()
    assert pool._bufs == {}
    c = pool.get("gn", 100)
    assert c is not b and c.numel() == 100


# ------------------------------------------------------------------------------------------------ the column-sums rule
def unet_rule_before(self, r_hw, layer, m, ln_next, kw, w_groups):
    """``SVDUNetHIP._gemm`` before the merge: its condition for ``gn_part``, clause for clause (``kw`` still holds
    ``gn_next``, as it did there)."""
    return bool(kw.pop("gn_next", False) and self.gn_from_epilogue and m % 256 == 0 and layer.n == layer.n_true
                and not layer.geglu and (layer.n % 320 == 0 or layer.n % 256 == 0) and r_hw % 256 == 0
                and layer.colsum is None and ln_next is None and "euler" not in kw and w_groups is None
                and (self.gn_epilogue_residual or (kw.get("res1") is None and kw.get("res2") is None)))


def vae_rule_before(self, layer, m, gn_rows):
    """``_VAEKernels._gemm`` before the merge."""
    n_store = layer.n_true if layer.n_true != layer.n else 0
    return bool(gn_rows and self.gn_from_epilogue and gn_rows % 256 == 0 and m % 256 == 0 and n_store == 0
                and (layer.n % 256 == 0 or layer.n % 320 == 0))


def engine(**switches):
    e = object.__new__(common._Engine)
    e.__dict__.update(switches)
    return e


def test_column_sums_rule_equals_both_rules_it_replaces():
    onoff = (False, True)
    engines = [engine(gn_from_epilogue=a, gn_epilogue_residual=b) for a in onoff for b in onoff]
    res, nxt, groups = object(), object(), (object(), object(), 256)
    points = granted = vae_points = 0
    for n in (64, 128, 192, 256, 320, 512, 640, 768):
        for n_true, geglu, fold in itertools.product(sorted({n, *(v for v in (4, 8) if v < n)}), onoff, onoff):
            layer = types.SimpleNamespace(n=n, n_true=n_true, geglu=geglu, colsum=object() if fold else None)
            for m, frame_rows, has_res, has_next, has_euler, has_groups, eng in itertools.product(
                    (255, 256, 512, 2016, 6144, 6400), (0, 64, 192, 256, 576, 1024), onoff, onoff, onoff, onoff, engines):
                epi = dict(r1scale=1.0)
                if has_res:
                    epi.update(res1=res)
                if has_euler:
                    epi.update(euler={})
                ln_next, w_groups = nxt if has_next else None, groups if has_groups else None
                got = eng._gn_part_ok(layer, m, frame_rows, epi, ln_next=ln_next, w_groups=w_groups)
                # the UNet asked with gn_next at a level of r.hw rows per frame: frame_rows = r.hw if gn_next else 0
                want = unet_rule_before(eng, frame_rows or 256, layer, m, ln_next, dict(epi, gn_next=frame_rows > 0), w_groups)
                assert got is want, (n, n_true, geglu, fold, m, frame_rows, epi, has_next, has_groups, eng.__dict__)
                points += 1
                granted += got
                # what a VAE can ask: plain layers, no ln_next, no Euler tail, no groups; it never refused behind a residual
                if not (geglu or fold or has_next or has_euler or has_groups) and eng.gn_epilogue_residual:
                    assert got is vae_rule_before(eng, layer, m, frame_rows), (n, n_true, m, frame_rows, has_res, eng.__dict__)
                    vae_points += 1
    assert points == (8 * 3 * 2 * 2) * (6 * 6) * 2 ** 4 * 4 and vae_points == (8 * 3) * (6 * 6) * 2 * 2
    assert 0 < granted < points


def test_a_second_residual_is_a_residual():
    """(``res2`` alone refuses the sums with the residual switch off, as ``res1`` does.)"""
    layer = types.SimpleNamespace(n=256, n_true=256, geglu=False, colsum=None)
    off, on = engine(gn_from_epilogue=True, gn_epilogue_residual=False), engine(gn_from_epilogue=True, gn_epilogue_residual=True)
    for epi in (dict(res2=object()), dict(res1=object(), res2=object())):
        assert not off._gn_part_ok(layer, 512, 256, epi) and on._gn_part_ok(layer, 512, 256, epi)
    assert off._gn_part_ok(layer, 512, 256, dict(res1=None, res2=None))


# ------------------------------------------------------------------------------------------------ the row-statistics rule
def ln_out_rule_before(self, layer, m):
    """``SVDUNetHIP._ln_out_ok`` before the merge."""
    if layer.n != layer.n_true or layer.geglu:
        return False
    return layer.n_true in (256, 320, 512, 640) or (self.ln_out_wide and layer.n_true in (768, 960, 1024, 1280)
                                                    and m > self.SPLITK_MAX_ROWS)


def test_row_statistics_rule_equals_the_rule_it_replaces():
    assert common._Engine.SPLITK_MAX_ROWS == 6144
    granted = 0
    for wide in (False, True):
        eng = engine(ln_out_wide=wide)
        for n, m, geglu, padded in itertools.product((256, 320, 512, 640, 768, 960, 1024, 1280, 1536),
                                                     (256, 6143, 6144, 6145, 6400, 16384), (False, True), (False, True)):
            layer = types.SimpleNamespace(n=n, n_true=n // 2 if geglu else n - 56 if padded else n, geglu=geglu)
            got = eng._ln_out_ok(layer, m)
            assert got is ln_out_rule_before(eng, layer, m), (wide, n, m, geglu, padded)
            assert got == (not geglu and not padded and (n <= 640 or (wide and n <= 1280 and m > 6144)))
            granted += got
    assert granted == 2 * 6 * 4 + 3 * 4     # one / two tiles at every m, either switch value; three / four from 6,145 rows
