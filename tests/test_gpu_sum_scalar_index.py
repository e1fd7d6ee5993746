"""The wide packed sum with its sample index on the scalar unit (sum_terms16w's quad shape, termdaw_amd/csrc/sum_index.h: packed
tables carry 255 wrap frames, a wave's start index, step and wrap are uniform, the load adds the lane's 16 bytes) against the
oracle, bit for bit: PCM, the f32 copy where kept, and the carried peak.

The timelines are the shortest that take the 16-frames-per-lane form by themselves: 58 s at 48 kHz, block 1 024 = 2 718.75 tiles
(the form starts at 2 600; the last tile is partial in every case here).  Over 2 719 blocks a loop length coprime to 1 024 puts
the loop's end at every lane of every quad.  Loop lengths: around every boundary of the form -- 1 .. 3 (the loop repeats inside
the pad), 254 .. 258 (the pad, the quad), 511 .. 513, 1 023 .. 1 025 (the wave's span), 4 095 / 4 097 (the workgroup's), 40 001.
Source counts 1, 2, 3, 4, 5, 7, 8: the tails of the batches of four.

Not covered: a second chunk (engine option max_chunk_frames) that still takes the wide form.  A chunk takes it from 2 600 tiles
on, 58 s hold 2 719: whatever the cap, at most one chunk of this timeline is long enough, and it starts at the cursor the
two-renders case below already has (a first chunk too short for the form, then a wide one, needs a timeline of twice the length)."""
import numpy as np
import pytest

from termdaw_amd import batch as tb
from termdaw_amd import workloads as W
from test_gpu_parity import assert_bit_exact, _bits

BENCH_OPTS = {"fuse_sources": 1, "packed_samples": 1, "output_f32": 0}   # bench.py build_batch()
SECONDS = 58.0
ALL_LENS = (1, 2, 3, 254, 255, 256, 257, 258, 511, 512, 513, 1023, 1024, 1025, 4095, 4097, 40001)
# every length at least once, every source count once
CASES = [
    (257,),
    (1, 40001),
    (2, 255, 1025),
    (3, 256, 1023, 4097),
    (255, 257, 1023, 1025, 4097),
    (254, 258, 511, 512, 513, 1024, 4095),
    (1, 3, 254, 256, 511, 513, 4095, 40001),
]


def test_the_cases_cover_every_length_and_source_count():
    assert {n for c in CASES for n in c} == set(ALL_LENS)
    assert sorted(len(c) for c in CASES) == [1, 2, 3, 4, 5, 7, 8]
    assert W.chunk_count(48000, SECONDS, 1024) * 1024 >= 2600 * 1024 and (48000 * int(SECONDS)) % 1024 != 0


def _project(lens, seconds=SECONDS, out="norm", bits24=()):
    """Looping sources of the given lengths into one Normalize (the fused single-pass form when it is the output) or one Sum."""
    p = W.ProjectScript(48000, 1024)
    p.set_length(seconds)
    p.set_render_samplerate(48000)
    p.set_render_bitdepth(16)
    for k, n in enumerate(lens):
        pcm = W.noise_int16(5200 + 31 * k + n, n)
        if k in bits24:
            pcm = pcm.astype(np.int32) * 256 + (k + 1)
        p.assets["s%d" % k] = W.Asset(pcm, bits=24 if k in bits24 else 16)
        p.load_sample("s%d" % k, "s%d" % k, "")
        p.add_sampleloop("v%d" % k, 0.4 + 0.15 * k, -70.0 + 20.0 * k, "s%d" % k)
    if out == "norm":
        p.add_normalize("sum", 1.0, 0.0)
    else:
        p.add_sum("sum", 0.8, 15.0)
    for k in range(len(lens)):
        p.connect("v%d" % k, "sum")
    p.set_output("sum")
    return p


def _render_pair(gpu_api, oracle, p, opts, renders=1, debug=0, groups=0, is_norm=True):
    """`renders` renders in a row WITHOUT rewinding the graph: the second starts at the cursor the first left (t0 = its frames)."""
    sb, fb, g = p.build(gpu_api)
    for k, v in opts.items():
        g.set_option(k, v)
    if groups:
        g.set_option("debug.sum_groups", groups)
    g.set_option("debug.norm", debug)
    osb, ofb, og = p.build(oracle)
    f32 = bool(opts.get("output_f32", 1))
    for rep in range(renders):
        fb.set_time(0)
        ofb.set_time(0)
        got = g.render_all(sb, fb, p.cs, 16, want_f32=f32)
        ref = og.render_all(osb, ofb, p.cs, 16, want_f32=f32)
        if f32:
            assert_bit_exact(got, ref)
        else:
            assert got[1] is None and np.array_equal(got[0], ref[0]), "render %d" % rep
        if is_norm:
            assert g.get_normalization_value("sum") == og.get_normalization_value("sum")
    return g


# ---- 1. loop lengths x source counts, the fused Normalize as the output vertex, both output forms ----
@pytest.mark.gpu
@pytest.mark.parametrize("lens", CASES, ids=lambda c: "n%d" % len(c))
def test_loop_lengths_and_source_counts(gpu_api, oracle, lens):
    p = _project(lens)
    g = _render_pair(gpu_api, oracle, p, BENCH_OPTS)
    assert g.norm_fix_runs() == 0
    _render_pair(gpu_api, oracle, p, dict(BENCH_OPTS, output_f32=1))


# ---- 2. a non-zero cursor ----
@pytest.mark.gpu
def test_two_renders_in_a_row_without_rewinding(gpu_api, oracle):
    """The second render's t0 is the first's 2 719 blocks: every source starts somewhere inside its loop, the peak is carried."""
    g = _render_pair(gpu_api, oracle, _project((3, 255, 257, 1025, 40001)), BENCH_OPTS, renders=2)
    assert g.norm_fix_runs() == 0


# ---- 3. the other outputs ----
@pytest.mark.gpu
def test_a_plain_sum_as_the_output(gpu_api, oracle):
    _render_pair(gpu_api, oracle, _project((2, 256, 513, 1023, 4097), out="sum"), dict(BENCH_OPTS, output_f32=1), is_norm=False)


@pytest.mark.gpu
def test_forced_give_up_redoes_the_vertex_from_the_stored_block_peaks(gpu_api, oracle):
    """debug.norm 1: every wait gives up at once; k_norm_fix scales the raw sums by the block peaks the launch stored."""
    g = _render_pair(gpu_api, oracle, _project((1, 254, 258, 1024, 4095)), dict(BENCH_OPTS, output_f32=1), renders=2, debug=1)
    assert g.norm_fix_runs() >= 1


@pytest.mark.gpu
def test_two_projects_through_the_batch(gpu_api, oracle):
    lens = [(255, 257, 1025), (1, 256, 511, 4097, 40001)]
    batch, first = tb.build_shard(gpu_api, lambda pid: _project(lens[pid]), [0, 1], dict(BENCH_OPTS))
    want_pcm, want_peak = [], []
    for pid in range(2):
        p = _project(lens[pid])
        osb, ofb, og = p.build(oracle)
        want_pcm.append(og.render_all(osb, ofb, p.cs, 16, want_f32=False)[0])
        want_peak.append(np.float32(og.get_normalization_value("sum")))
    cs = first.cs
    batch.rewind()
    assert batch.render_all(cs, 16) == cs * 1024
    for i in range(2):
        assert np.array_equal(batch.read_pcm(i, cs), want_pcm[i]), "project %d" % i
    assert np.array_equal(_bits(batch.peaks()), _bits(np.array(want_peak, np.float32)))


# ---- 4. the ragged form shares the template ----
@pytest.mark.gpu
@pytest.mark.parametrize("G", [13, 40])
def test_the_ragged_form_on_one_second(gpu_api, oracle, G):
    """188 quads over 13 workgroups (waves of 3 and 4 quads) and over 40 (waves of 1 and 2): every body of the shared template."""
    p = _project((255, 256, 257, 1000), seconds=1.0)
    _render_pair(gpu_api, oracle, p, BENCH_OPTS, groups=G, renders=2)
    _render_pair(gpu_api, oracle, p, dict(BENCH_OPTS, output_f32=1), groups=G)


@pytest.mark.gpu
def test_the_ragged_form_at_full_length(gpu_api, oracle):
    """The shared template on the 58 s timeline whatever launch_sum's thresholds for the automatic choice are: debug.sum_groups
    704 forces k_sum16r with 10 875 quads over 704 workgroups (15 or 16 each: waves of 3 and 4 quads)."""
    _render_pair(gpu_api, oracle, _project((3, 255, 257, 1025, 40001)), BENCH_OPTS, groups=704, renders=2)


# ---- 5. the other readers of the padded tables ----
@pytest.mark.gpu
def test_a_24_bit_asset_beside_16_bit_ones(gpu_api, oracle):
    """The 24-bit asset has no packed twin: the launch falls to the mixed form, which reads the 16-bit sources' padded tables
    with a modulo per lane, as before."""
    p = _project((255, 4097, 1023, 3), bits24=(1,))
    _render_pair(gpu_api, oracle, p, dict(BENCH_OPTS, output_f32=1))
    _render_pair(gpu_api, oracle, _project((255, 4097, 1023, 3), seconds=1.0, bits24=(1,)), BENCH_OPTS, renders=2)
