"""``spatial_window`` without a GPU: which levels of the benchmark latent record ``attn_spatial_window`` and with what, that
nothing records it when the option is absent, and the command-line switch of the two modes."""
import collections

import pytest

from tests.test_launch_plan_cpu import BENCH_LATENT, SPATIAL_ATTENTION, log, run_unet      # noqa: F401  (log: the fixture)


def spatial(log):
    """tokens per frame -> Counter of the spatial-attention wrappers recorded at that level"""
    seen = collections.defaultdict(collections.Counter)
    for l in log:
        if l.name in SPATIAL_ATTENTION + ("attn_spatial_window",):
            hw = l.kw["h"] * l.kw["w"] if l.name == "attn_spatial_window" else l.kw["seq_q"] if l.name == "attn_spatial_kv" else l.kw["seq"]
            seen[hw][l.name] += 1
    return dict(seen)


def test_window_route_takes_level_0_of_the_benchmark_latent_and_nothing_else(log):
    """72 x 128 divides by 8 and has 9,216 tokens; 36 x 64 does not divide, the coarser levels are below the threshold."""
    b, f = BENCH_LATENT[:2]
    run_unet(log, 64, BENCH_LATENT)
    base = spatial(log)
    assert not any(l.name == "attn_spatial_window" for l in log)
    run_unet(log, 64, BENCH_LATENT, spatial_window=(5, 7))
    got = spatial(log)
    assert got[9216] == {"attn_spatial_window": 5} and {hw: n for hw, n in got.items() if hw != 9216} == {hw: n for hw, n in base.items() if hw != 9216}
    for l in log:
        if l.name == "attn_spatial_window":
            assert (l.kw["h"], l.kw["w"], l.kw["wh"], l.kw["ww"], l.kw["batch"]) == (72, 128, 5, 7, b * f)
            assert l.kw["ldq"] == l.kw["ldk"] == l.kw["ldv"] == 3 * l.kw["ldo"] == 3 * 64 * l.kw["heads"]


def test_window_route_from_the_environment_and_below_the_threshold(log, monkeypatch):
    monkeypatch.setenv("VDPP_SPATIAL_WINDOW", "3,3")
    hip = run_unet(log, 64, (1, 2, 8, 16, 24), spatial_window_min_tokens=1)
    assert hip.spatial_window == (3, 3)
    assert spatial(log)[384] == {"attn_spatial_window": 5} and sum(l.name == "attn_spatial_window" for l in log) == 5
    run_unet(log, 64, (1, 2, 8, 16, 24))                                   # 384 tokens < 4,096
    assert not any(l.name == "attn_spatial_window" for l in log)


@pytest.mark.parametrize("mode,argv", [("generate", ["--input-image", "a.png", "--output", "a.gif", "--random-init"]), ("production", [])])
def test_command_line_switch(mode, argv):
    import importlib
    parse = importlib.import_module(f"vdpp_amd.modes.{mode}").parse_args
    assert parse(argv).spatial_window is None
    assert tuple(parse(argv + ["--spatial-window", "5", "7"]).spatial_window) == (5, 7)
