"""The wide packed sum's single-pass Normalize with the EARLY store (k_sum16w, SumDesc modes 4 / 5): a tile looks once at
the lower tiles' published peaks, scales / quantises / stores with the running peak it can see, only then waits for the rest, and
stores again every block whose running peak came out differently (termdaw_amd/csrc/sum_runmax.h) -- against the oracle, bit for
bit: PCM, the f32 copy where kept, and the carried peak.

Engine option debug.norm: bit 0 every wait gives up at once (k_norm_fix redoes the vertex), bit 2 the look sees nothing (every tile
stores with its own peaks first: the store-again path runs deterministically), bit 3 the other order of store and wait than the
default (read-only option debug.norm_early_store says which the default is), bit 4 only counts.  Every setting below is run as named
AND with the early store switched on explicitly, whichever order is the default.

Timelines as in tests/test_gpu_sum_scalar_index.py: 58 s at 48 kHz, block 1 024 = 2 719 blocks in 680 tiles of four, the last tile
partial.  "rising": one source as long as the timeline, |x| = 1000 + 10 * block with alternating sign -- every block is a new record,
so a block's own peak IS its running peak and nothing is stored twice whatever a tile saw.  "falling": the same reversed -- block 0
is the record, and a tile that saw nothing stores every block twice (all but tile 0's four, which has nothing to wait for).
The oracle's renders are made once per project and shared."""
import functools

import numpy as np
import pytest

from termdaw_amd import batch as tb
from termdaw_amd import workloads as W
from test_gpu_parity import _bits
from test_gpu_sum_scalar_index import BENCH_OPTS, SECONDS, _project

CS = W.chunk_count(48000, SECONDS, 1024)
NOISE_LENS = (3, 255, 257, 1025, 40001)
B0, B2, B3, B4 = 1, 4, 8, 16


def _ramp_project(falling):
    blk = np.arange(CS, dtype=np.int64)
    v = (1000 + 10 * blk) * np.where(blk % 2 == 0, 1, -1)
    if falling:
        v = v[::-1]
    pcm = np.repeat(v, 1024).astype(np.int16)
    p = W.ProjectScript(48000, 1024)
    p.set_length(SECONDS)
    p.set_render_samplerate(48000)
    p.set_render_bitdepth(16)
    p.assets["ramp"] = W.Asset(np.stack([pcm, pcm], axis=1))
    p.load_sample("ramp", "ramp", "")
    p.add_sampleloop("v0", 0.7, -20.0, "ramp")
    p.add_normalize("sum", 1.0, 0.0)
    p.connect("v0", "sum")
    p.set_output("sum")
    return p


def _make(name):
    return _ramp_project(name == "falling") if name in ("rising", "falling") else _project(NOISE_LENS)


@functools.lru_cache(maxsize=None)
def _reference(oracle, name, renders):
    """[(pcm, f32, carried peak)] of `renders` renders in a row without rewinding the graph -- made once, never written to."""
    p = _make(name)
    osb, ofb, og = p.build(oracle)
    out = []
    for _ in range(renders):
        ofb.set_time(0)
        pcm, f = og.render_all(osb, ofb, p.cs, 16, want_f32=True)
        pcm.setflags(write=False)
        f.setflags(write=False)
        out.append((pcm, f, og.get_normalization_value("sum")))
    return out


def _check(gpu_api, oracle, name, debug, f32=0, renders=1):
    """Renders `name` with debug.norm `debug`; returns (graph, blocks stored twice per render)."""
    p = _make(name)
    assert p.cs == CS and CS == 2719
    sb, fb, g = p.build(gpu_api)
    for k, v in dict(BENCH_OPTS, output_f32=f32).items():
        g.set_option(k, v)
    g.set_option("debug.norm", debug)
    again = []
    for rep, (rpcm, rf, rpeak) in enumerate(_reference(oracle, name, renders)):
        fb.set_time(0)
        pcm, f = g.render_all(sb, fb, p.cs, 16, want_f32=bool(f32))
        assert np.array_equal(pcm, rpcm), "%s debug %d render %d: PCM" % (name, debug, rep)
        if f32:
            assert np.array_equal(_bits(f), _bits(rf)), "%s debug %d render %d: f32" % (name, debug, rep)
        else:
            assert f is None
        assert g.get_normalization_value("sum") == rpeak
        again.append(g.norm_respec())
    return g, again


def _early(gpu_api):
    """debug.norm bits that switch the early store ON whatever the default order is."""
    g = gpu_api.Graph(1024, 48000)
    return 0 if g.get_option("debug.norm_early_store") else B3


def _settings(gpu_api, *values):
    """The settings as named, and each with the early store on explicitly (duplicates dropped)."""
    on = _early(gpu_api)
    return sorted({v for v in values} | {(v & ~B3) | on for v in values})


def _early_is_on(gpu_api, debug):
    return ((debug & B3) != 0) != (_early(gpu_api) == 0)


@pytest.mark.gpu
def test_rising_every_block_a_new_record_nothing_is_stored_twice(gpu_api, oracle):
    for debug in _settings(gpu_api, 0, B2, B3):
        g, again = _check(gpu_api, oracle, "rising", debug | B4)
        assert again == [0] and g.norm_fix_runs() == 0, debug


@pytest.mark.gpu
def test_falling_block_0_is_the_record_every_other_tile_stores_twice(gpu_api, oracle):
    for debug in _settings(gpu_api, B2):
        g, again = _check(gpu_api, oracle, "falling", debug)
        assert again == [CS - 4 if _early_is_on(gpu_api, debug) else 0] and g.norm_fix_runs() == 0, debug
    # (as the dispatcher orders the tiles: whatever was stored twice, at most the blocks of the tiles that had to wait)
    g, again = _check(gpu_api, oracle, "falling", _early(gpu_api) | B4)
    assert 0 <= again[0] <= CS - 4 and g.norm_fix_runs() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("f32", [0, 1])
def test_noise_both_output_forms(gpu_api, oracle, f32):
    for debug in _settings(gpu_api, 0, B2):
        g, again = _check(gpu_api, oracle, "noise", debug, f32=f32)
        assert g.norm_fix_runs() == 0, debug
        if not (debug & B2) or not _early_is_on(gpu_api, debug):
            assert again == [0], debug   # (not counted / nothing stored early)


@pytest.mark.gpu
def test_two_renders_in_a_row_the_second_from_a_carried_max(gpu_api, oracle):
    for debug in _settings(gpu_api, 0):
        g, _ = _check(gpu_api, oracle, "noise", debug, renders=2)
        assert g.norm_fix_runs() == 0, debug


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["noise", "rising"])
def test_forced_give_up_overwrites_whatever_was_stored(gpu_api, oracle, name):
    for debug in _settings(gpu_api, B0, B0 | B2):
        g, _ = _check(gpu_api, oracle, name, debug, f32=1)
        assert g.norm_fix_runs() == 1, debug


@pytest.mark.gpu
def test_three_projects_through_the_batch(gpu_api, oracle):
    """Words and counters are per project (blockIdx.y): rising stores nothing twice, falling everything but tile 0, noise what it
    stores alone."""
    names = ["rising", "falling", "noise"]
    for debug in _settings(gpu_api, 0, B2):
        batch, first = tb.build_shard(gpu_api, lambda pid: _make(names[pid]), [0, 1, 2], dict(BENCH_OPTS, **{"debug.norm": debug}))
        batch.rewind()
        assert batch.render_all(first.cs, 16) == CS * 1024
        for i, name in enumerate(names):
            rpcm, _, rpeak = _reference(oracle, name, 1)[0]
            assert np.array_equal(batch.read_pcm(i, CS), rpcm), "project %d (%s), debug %d" % (i, name, debug)
        want = np.array([_reference(oracle, n, 1)[0][2] for n in names], np.float32)
        assert np.array_equal(_bits(batch.peaks()), _bits(want))
        again = batch.projects[0][2].norm_respec()
        if debug & B2 and _early_is_on(gpu_api, debug):
            assert again == 0 + (CS - 4) + _check(gpu_api, oracle, "noise", debug)[1][0], debug
        else:
            assert again == 0, debug
