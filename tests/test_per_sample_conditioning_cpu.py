"""Per-sample conditioning through the pipeline stage (``run_many(..., conditioning_supplier=)``) on CPU ranks.

A stub model whose step depends on its ``conditioning`` runs over Gloo through the chain, the rotating chain and the ring,
with one and two interleave lanes: every sample on the finishing rank must equal the plain loop with that sample's own
conditioning, bit for bit; every rank calls the supplier once per sample it steps, and the conditioning never adds a
message (the per-rank point-to-point sequence is the one of a run without a supplier)."""

import logging
import math
import os
import tempfile
import threading

import pytest
import torch
import torch.multiprocessing as mp

from vdpp_amd.distributed import finalize_distributed, init_distributed
from vdpp_amd.models import DummyUNet
from vdpp_amd.pipeline import LatentSpec, PipelineConfig, PipelineStage, run_pipeline_latents

SHAPE = (1, 4, 2, 4, 6)


class CondStub(torch.nn.Module):
    """``latent * (1 - 0.01 * a) + b * sin(step + 1)`` with (a, b) = the call's conditioning."""

    def forward(self, latent, step, conditioning=None):
        if conditioning is None:
            raise AssertionError("the stage dropped the conditioning")
        a, b = conditioning
        return latent * (1.0 - 0.01 * a) + b * math.sin(step + 1.0)


def _cond(i):
    return (1.0 + 0.5 * (i % 3), 0.1 * i - 0.3)        # distinct per sample: a sample stepped with another's is caught


def _input(i):
    g = torch.Generator().manual_seed(1000 + i)
    return torch.randn(SHAPE, generator=g)


def _plain(i, timesteps):
    lat, model = _input(i), CondStub()
    for s in timesteps:
        lat = model(lat, s, conditioning=_cond(i))
    return lat


def _config(ws, rank, total_steps, mode, conc):
    spec = LatentSpec(shape=torch.Size(SHAPE), dtype=torch.float32, device=torch.device("cpu"))
    return PipelineConfig(total_steps=total_steps, world_size=ws, rank=rank, timesteps=list(reversed(range(total_steps))),
                          latent_spec=spec, balanced=True, ring=mode == "ring", rotate=mode == "rotate",
                          concurrent_samples=conc)


def _worker(rank, ws, init_file, out_dir, num_samples, total_steps, mode, conc):
    torch.set_num_threads(1)
    init_distributed(backend="gloo", rank=rank, world_size=ws, init_method=f"file://{init_file}")
    quiet = logging.getLogger("quiet"); quiet.setLevel(logging.ERROR)
    stage = PipelineStage(CondStub(), _config(ws, rank, total_steps, mode, conc), logger=quiet)
    calls = []

    def conditioning_supplier(i):
        calls.append(i)
        return _cond(i)

    with torch.no_grad():
        outs = stage.run_many(num_samples, input_supplier=_input if (mode == "ring" or rank == 0) else None,
                              conditioning_supplier=conditioning_supplier)
    torch.save({"calls": calls, "outs": outs}, os.path.join(out_dir, f"rank{rank}.pt"))
    finalize_distributed()


@pytest.mark.parametrize("ws,num_samples,total_steps,mode,conc", [
    (2, 5, 7, "chain", 1),
    (3, 7, 7, "chain", 2),
    (4, 6, 9, "rotate", 1),
    (3, 5, 7, "rotate", 2),
    (2, 5, 7, "ring", 1),
    (3, 7, 7, "ring", 2),
    (4, 9, 9, "ring", 2),
    (8, 32, 25, "ring", 2),      # the 8-rank configuration of the real-size schedule tests: 25 steps, 32 samples
])
def test_gloo_schedules_with_per_sample_conditioning_equal_plain_loop(ws, num_samples, total_steps, mode, conc):
    with tempfile.TemporaryDirectory() as td:
        mp.spawn(_worker, args=(ws, os.path.join(td, "init"), td, num_samples, total_steps, mode, conc), nprocs=ws,
                 join=True)
        got = [torch.load(os.path.join(td, f"rank{r}.pt")) for r in range(ws)]
    for r in range(ws):
        # every rank owns a share of every sample (balanced splits give each rank >= 1 step): one call per sample
        assert sorted(got[r]["calls"]) == list(range(num_samples)), f"rank {r} supplier calls {got[r]['calls']}"
        if r < ws - 1:
            assert got[r]["outs"] is None
    outs = got[ws - 1]["outs"]
    assert len(outs) == num_samples
    ts = list(reversed(range(total_steps)))
    for i, lat in enumerate(outs):
        assert torch.equal(lat, _plain(i, ts)), f"sample {i}"


def test_supplier_called_before_the_first_local_step_and_released_after():
    """One rank: the supplier runs before the sample's first step, once, and the stage keeps no reference afterwards."""
    import gc
    import weakref

    events, refs = [], []

    class Cond:
        def __init__(self, i):
            self.i = i

    class Model(torch.nn.Module):
        def forward(self, latent, step, conditioning=None):
            events.append(("step", conditioning.i, step))
            return latent + conditioning.i

    def supplier(i):
        events.append(("supply", i))
        c = Cond(i)
        refs.append(weakref.ref(c))
        return c

    stage = PipelineStage(Model(), _config(1, 0, 3, "chain", 1))
    outs = stage.run_many(2, input_supplier=lambda i: torch.zeros(SHAPE), conditioning_supplier=supplier)
    assert events == [("supply", 0), ("step", 0, 2), ("step", 0, 1), ("step", 0, 0),
                      ("supply", 1), ("step", 1, 2), ("step", 1, 1), ("step", 1, 0)]
    assert [float(o.flatten()[0]) for o in outs] == [0.0, 3.0]
    gc.collect()
    assert all(r() is None for r in refs), "the stage still holds a sample's conditioning"


def test_without_supplier_the_model_is_called_as_before():
    z_model = DummyUNet(4, 16).eval()
    stage = PipelineStage(z_model, _config(1, 0, 3, "chain", 1))
    x = torch.randn(SHAPE)
    with torch.no_grad():
        outs = stage.run_many(2, input_supplier=lambda i: x * (i + 1))
        want = x * 2
        for s in (2, 1, 0):
            want = z_model(want, s)
    assert torch.equal(outs[1], want)


def test_supplier_with_a_model_without_the_keyword_is_refused_before_any_communication():
    # rank 1 of 2 with no process group: anything that reached the transport would fail differently
    for mode in ("chain", "rotate", "ring"):
        stage = PipelineStage(DummyUNet(4, 16), _config(2, 1, 7, mode, 1))
        with pytest.raises(ValueError, match="conditioning"):
            stage.run_many(3, input_supplier=_input, conditioning_supplier=_cond)
    with pytest.raises(ValueError, match="conditioning"):
        run_pipeline_latents(DummyUNet(4, 16), total_steps=3, timesteps=[2, 1, 0], world_size=1, rank=0,
                             latent_spec=LatentSpec(torch.Size(SHAPE), torch.float32, torch.device("cpu")), num_samples=1,
                             input_supplier=_input, conditioning_supplier=_cond)


def test_run_pipeline_latents_passes_the_supplier():
    spec = LatentSpec(shape=torch.Size(SHAPE), dtype=torch.float32, device=torch.device("cpu"))
    outs = run_pipeline_latents(CondStub(), total_steps=4, timesteps=[3, 2, 1, 0], world_size=1, rank=0, latent_spec=spec,
                                num_samples=3, input_supplier=_input, conditioning_supplier=_cond)
    for i, lat in enumerate(outs):
        assert torch.equal(lat, _plain(i, [3, 2, 1, 0]))


def _threads_as_ranks(world, fn, timeout=120):
    results, errors = {}, []

    def main(rank):
        try:
            results[rank] = fn(rank)
        except Exception as exc:       # noqa: BLE001  (reported in the main thread)
            errors.append((rank, repr(exc)))

    ts = [threading.Thread(target=main, args=(r,)) for r in range(world)]
    for t in ts: t.start()
    for t in ts: t.join(timeout=timeout)
    assert all(not t.is_alive() for t in ts), f"a rank is stuck; errors so far: {errors}"
    return results, errors


@pytest.mark.parametrize("world,num_samples,conc,mode", [(2, 5, 1, "ring"), (3, 7, 2, "ring"), (4, 9, 2, "ring"),
                                                        (3, 5, 1, "rotate"), (4, 6, 1, "chain")])
def test_supplier_adds_no_message_under_pair_fifo_rules(monkeypatch, world, num_samples, conc, mode):
    """Under the RCCL pair-FIFO emulation (tests/p2p_emulation.py) the per-rank sequence of sends and receives with a
    conditioning supplier is exactly the one without (the conditioning is made on every rank, never sent)."""
    import vdpp_amd.pipeline.pipeline as pl
    from tests.p2p_emulation import PairFifoTransport

    total_steps = 9

    def run(with_supplier):
        net = PairFifoTransport(timeout=60)
        with monkeypatch.context() as mctx:
            net.install(mctx, pl.dist)

            def rank_main(rank):
                net.bind(rank)
                quiet = logging.getLogger("quiet"); quiet.setLevel(logging.ERROR)
                if with_supplier:
                    model, kw = CondStub(), dict(conditioning_supplier=_cond)
                else:
                    model, kw = (lambda lat, step: CondStub()(lat, step, conditioning=(1.0, 0.0))), {}
                stage = PipelineStage(model, _config(world, rank, total_steps, mode, conc), logger=quiet)
                with torch.no_grad():
                    return stage.run_many(num_samples, input_supplier=_input if (mode == "ring" or rank == 0) else None,
                                          **kw)

            results, errors = _threads_as_ranks(world, rank_main)
        assert not errors, errors
        assert net.crossed is None and net.idle()
        return results, [[(k, p) for r, k, p in net.log if r == rank] for rank in range(world)]

    plain_out, plain_seq = run(False)
    cond_out, cond_seq = run(True)
    assert cond_seq == plain_seq
    ts = list(reversed(range(total_steps)))
    outs = cond_out[world - 1]
    assert len(outs) == num_samples
    for i, lat in enumerate(outs):
        assert torch.equal(lat, _plain(i, ts)), f"sample {i}"


def test_production_cli_takes_per_sample_motion_buckets():
    from vdpp_amd.modes.production import parse_args

    assert parse_args([]).sample_motion_buckets is None
    assert parse_args(["--sample-motion-buckets", "10", "200", "127"]).sample_motion_buckets == [10, 200, 127]
