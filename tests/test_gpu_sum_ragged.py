"""The ragged form of the wide packed sum (k_sum16r, DESIGN.md section 2: quads of 256 frames dealt evenly over a grid that fills
every CU alike) against the oracle, bit for bit: PCM, the f32 copy where kept, and the carried peak.  Engine option
debug.sum_groups forces the form -- and its grid -- on one-second config-2 projects (47 blocks = 188 quads) with bench.py's
options, so that every wave size (1 .. 4 quads), every boundary kind (block-aligned, straddled), the source-count tails, short
loops, the wait for the NEXT workgroup's head granule, the carried peak, the forced give-up (k_norm_fix from the two-slot block
peaks), the other outputs and the batch path are reached in a few milliseconds each."""
import numpy as np
import pytest

from termdaw_amd import batch as tb
from termdaw_amd import workloads as W
from test_gpu_parity import assert_bit_exact, _bits

BENCH_OPTS = {"fuse_sources": 1, "packed_samples": 1, "output_f32": 0}   # bench.py build_batch()
Q1 = 188                                                                  # quads of one second


def _groups(G, Q=Q1):
    return [(g * Q // G, (g + 1) * Q // G) for g in range(G)]


def _check(gpu_api, oracle, p, G, opts=BENCH_OPTS, renders=1, debug=0, reset=False):
    sb, fb, g = p.build(gpu_api)
    for k, v in opts.items():
        g.set_option(k, v)
    g.set_option("debug.sum_groups", G)
    g.set_option("debug.norm", debug)
    osb, ofb, og = p.build(oracle)
    f32 = bool(opts.get("output_f32", 1))
    for rep in range(renders):
        if reset:
            g.reset_normalize_vertices()
            og.reset_normalize_vertices()
        fb.set_time(0)
        ofb.set_time(0)
        got = g.render_all(sb, fb, p.cs, 16, want_f32=f32)
        ref = og.render_all(osb, ofb, p.cs, 16, want_f32=f32)
        if f32:
            assert_bit_exact(got, ref)
        else:
            assert got[1] is None and np.array_equal(got[0], ref[0]), "render %d, G = %d" % (rep, G)
        assert g.get_normalization_value("sum") == og.get_normalization_value("sum")
    return g


# ---- 1. every wave size and every boundary kind ----
def test_the_grids_cover_every_wave_size_and_boundary_kind():
    """(what the cases below rely on, from the partition's own formula)"""
    def waves(G):
        return {(w + 1) * (b - a) // 4 - w * (b - a) // 4 for a, b in _groups(G) for w in range(4)}
    def straddles(G):
        return [b for _, b in _groups(G)[:-1] if b % 4]
    assert {b - a for a, b in _groups(47)} == {4} and waves(47) == {1} and not straddles(47)
    assert {b - a for a, b in _groups(40)} == {4, 5} and waves(40) == {1, 2} and straddles(40)
    assert {b - a for a, b in _groups(13)} == {14, 15} and waves(13) == {3, 4} and straddles(13)
    assert {b - a for a, b in _groups(12)} == {15, 16} and waves(12) == {3, 4}


@pytest.mark.gpu
@pytest.mark.parametrize("G", [47, 40, 13, 12])
def test_one_second_on_every_kind_of_grid(gpu_api, oracle, G):
    _check(gpu_api, oracle, W.config2(seconds=1.0), G)


@pytest.mark.gpu
@pytest.mark.parametrize("G", [11, 48])
def test_a_grid_that_cannot_carry_the_quads_is_refused(gpu_api, G):
    p = W.config2(seconds=1.0, n_src=4)
    sb, fb, g = p.build(gpu_api)
    for k, v in BENCH_OPTS.items():
        g.set_option(k, v)
    g.set_option("debug.sum_groups", G)
    with pytest.raises(gpu_api.TermdawError, match="sum_groups"):
        g.render_all(sb, fb, p.cs, 16, want_f32=False)


# ---- 2. source-count tails: tail only, one batch, batch + tail, two batches + tail ----
@pytest.mark.gpu
@pytest.mark.parametrize("n_src", [3, 4, 5, 9])
def test_source_count_tails(gpu_api, oracle, n_src):
    _check(gpu_api, oracle, W.config2(seconds=1.0, n_src=n_src), 13)
    _check(gpu_api, oracle, W.config2(seconds=1.0, n_src=n_src), 40)


# ---- 3. loops shorter than a quad and shorter than a wave's span ----
@pytest.mark.gpu
@pytest.mark.parametrize("G", [40, 13])
def test_short_loops(gpu_api, oracle, G):
    p = W.config2(seconds=1.0, n_src=2, base_len=37)
    assert sorted(len(a.pcm) for a in p.assets.values()) == [37, 1014]
    _check(gpu_api, oracle, p, G)


# ---- 4. the wait for the next workgroup's head granule matters ----
FWD_G, FWD_SEED = 40, 3


def _raw_sum(oracle, seed_offset, seconds=1.0, n_src=64):
    """config 2's sources into a plain Sum vertex (gain 1, centre: the raw sum the Normalize vertex sees), on the CPU."""
    p = W.config2(seconds=seconds, n_src=n_src, seed_offset=seed_offset)
    q = W.ProjectScript(48000, 1024)
    q.set_length(seconds)
    q.set_render_samplerate(48000)
    q.set_render_bitdepth(16)
    q.assets = dict(p.assets)
    for k in range(n_src):
        q.load_sample("s%02d" % k, "s%02d" % k, "")
    for k in range(n_src):
        gain = float(np.float32(0.5) + np.float32(k) / np.float32(64.0))
        angle = float(np.float32(-90.0) + np.float32(180.0) * np.float32(k) / np.float32(max(n_src - 1, 1)))
        q.add_sampleloop("vs%02d" % k, gain, angle, "s%02d" % k)
    q.add_sum("sum", 1.0, 0.0)
    for k in range(n_src):
        q.connect("vs%02d" % k, "sum")
    q.set_output("sum")
    osb, ofb, og = q.build(oracle)
    return og.render_all(osb, ofb, q.cs, 16)[1]


def _forward_records(raw, G):
    """Straddled blocks whose record-setting peak lies in the LATER workgroup's quads: [(block, earlier part, later part, running before)]."""
    quad = np.abs(raw.reshape(-1, 256 * 2)).max(axis=1)
    run = np.maximum.accumulate(quad.reshape(-1, 4).max(axis=1))
    out = []
    for _, end in _groups(G, len(quad))[:-1]:
        if end % 4:
            b = end // 4
            early, late, before = quad[4 * b:end].max(), quad[end:4 * b + 4].max(), (run[b - 1] if b else 0.0)
            if late > early and late > before:
                out.append((b, float(early), float(late), float(before)))
    return out


def test_the_seed_puts_a_record_behind_a_straddle(oracle):
    """The precondition of the case below, on the CPU: a kernel that ignored the head granule would scale the earlier workgroup's
    quads of that block by the wrong peak."""
    rec = _forward_records(_raw_sum(oracle, FWD_SEED), FWD_G)
    assert rec, "no straddled block of seed %d sets its record in the later workgroup" % FWD_SEED


@pytest.mark.gpu
def test_a_record_in_the_later_part_of_a_straddled_block(gpu_api, oracle):
    assert _forward_records(_raw_sum(oracle, FWD_SEED), FWD_G)
    _check(gpu_api, oracle, W.config2(seconds=1.0, seed_offset=FWD_SEED), FWD_G)
    _check(gpu_api, oracle, W.config2(seconds=1.0, seed_offset=FWD_SEED), FWD_G, opts=dict(BENCH_OPTS, output_f32=1))


# ---- 5. carry and fallback ----
@pytest.mark.gpu
@pytest.mark.parametrize("G", [40, 13])
def test_the_running_peak_carries_over(gpu_api, oracle, G):
    g = _check(gpu_api, oracle, W.config2(seconds=1.0, seed_offset=FWD_SEED), G, renders=2)
    assert g.norm_fix_runs() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("G", [40, 13])
def test_forced_give_up_redoes_the_vertex_from_the_two_slot_block_peaks(gpu_api, oracle, G):
    """debug.norm 1: every wait gives up at once; k_norm_fix folds both contributors of a straddled block."""
    assert [b for _, b in _groups(G)[:-1] if b % 4]
    g = _check(gpu_api, oracle, W.config2(seconds=1.0, seed_offset=FWD_SEED), G, renders=2, debug=1, opts=dict(BENCH_OPTS, output_f32=1))
    assert g.norm_fix_runs() >= 1
    g = _check(gpu_api, oracle, W.config2(seconds=1.0, seed_offset=FWD_SEED), G, renders=2, debug=1, reset=True)
    assert g.norm_fix_runs() >= 1


# ---- 6. other outputs ----
@pytest.mark.gpu
@pytest.mark.parametrize("G", [40, 12])
def test_the_f32_copy(gpu_api, oracle, G):
    _check(gpu_api, oracle, W.config2(seconds=1.0, n_src=9), G, opts=dict(BENCH_OPTS, output_f32=1))


@pytest.mark.gpu
@pytest.mark.parametrize("G", [40, 13])
def test_a_plain_sum_vertex_feeding_a_normalize(gpu_api, oracle, G):
    """Mode 0: two Sum vertices of packed loops (the ragged form, pan and gain applied) into a Normalize vertex that reads their buffers."""
    n_src = 6
    src = W.config2(seconds=1.0, n_src=n_src)
    p = W.ProjectScript(48000, 1024)
    p.set_length(1.0)
    p.set_render_samplerate(48000)
    p.set_render_bitdepth(16)
    p.assets = dict(src.assets)
    for k in range(n_src):
        p.load_sample("s%02d" % k, "s%02d" % k, "")
        p.add_sampleloop("v%02d" % k, 0.5 + k / 8.0, -60.0 + 24.0 * k, "s%02d" % k)
    p.add_sum("a", 0.75, -20.0)
    p.add_sum("b", 1.25, 35.0)
    p.add_normalize("sum", 1.0, 0.0)
    for k in range(n_src):
        p.connect("v%02d" % k, "a" if k < 5 else "b")
    p.connect("v00", "b")
    p.connect("v01", "b")
    p.connect("a", "sum")
    p.connect("b", "sum")
    p.set_output("sum")
    _check(gpu_api, oracle, p, G, opts=dict(BENCH_OPTS, output_f32=1))


# ---- 7. batch ----
@pytest.mark.gpu
def test_three_projects_through_the_batch(gpu_api, oracle):
    n = 3
    batch, first = tb.build_shard(gpu_api, lambda pid: W.config2(seconds=1.0, seed_offset=64 * pid), list(range(n)),
                                  dict(BENCH_OPTS, **{"debug.sum_groups": 13}))
    want_pcm, want_peak = [], []
    for pid in range(n):
        p = W.config2(seconds=1.0, seed_offset=64 * pid)
        osb, ofb, og = p.build(oracle)
        want_pcm.append(og.render_all(osb, ofb, p.cs, 16, want_f32=False)[0])
        want_peak.append(np.float32(og.get_normalization_value("sum")))
    cs = first.cs
    for _ in range(2):
        batch.rewind()
        assert batch.render_all(cs, 16) == cs * 1024
        for i in range(n):
            assert np.array_equal(batch.read_pcm(i, cs), want_pcm[i]), "project %d" % i
        assert np.array_equal(_bits(batch.peaks()), _bits(np.array(want_peak, np.float32)))
