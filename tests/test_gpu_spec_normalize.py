"""Speculative single-pass normalize (SumDesc mode 3 + k_norm_fix): after Graph::true_normalize_scan
(graph.rs:222-237) the carried max is the scanned peak, so a render scales every block by 1 / max in the summing
kernel itself; k_norm_fix redoes the vertex the two-pass way when a block peak exceeds the carried max after all
(running max `*max = buf_max.max(*max)`, extensions.rs:323-328).  Both outcomes must equal the oracle bit for bit."""
import numpy as np
import pytest

from termdaw_amd import workloads as W
from test_gpu_parity import assert_bit_exact, assert_close

pytestmark = pytest.mark.gpu


def _profiled(g, render):
    g.set_profiling(1)
    out = render()
    names = set(g.kernel_times())
    g.set_profiling(0)
    return out, names


@pytest.mark.parametrize("spec,single", [(1, 1), (1, 0), (0, 1)])
def test_scanned_render_takes_the_single_pass(gpu_api, oracle, spec, single):
    p = W.config2(seconds=2.0)
    sb, fb, g = p.build(gpu_api)
    osb, ofb, og = p.build(oracle)
    g.set_option("debug.spec_normalize", spec)
    g.set_option("debug.single_pass_normalize", single)
    fresh_two_pass = not (spec and single)
    got, fam = _profiled(g, lambda: g.render_all(sb, fb, p.cs, 16))
    # un-scanned: the running peak -- in ONE launch (k_norm1 / k_sum16w mode 5: the grid is resident at once, the tiles hand
    # their maxima over through granules) or, with that switched off, the two passes k_sum + k_scale
    assert ("k_scale" in fam) == fresh_two_pass and "k_norm_fix" not in fam
    assert_bit_exact(got, og.render_all(osb, ofb, p.cs, 16))
    g.true_normalize_scan(sb, fb, p.cs)
    og.true_normalize_scan(osb, ofb, p.cs)
    for _ in range(2):
        got, fam = _profiled(g, lambda: g.render_all(sb, fb, p.cs, 16))
        assert ("k_norm_fix" in fam and "k_scale" not in fam) if spec else ("k_scale" in fam and "k_norm_fix" not in fam)
        assert_bit_exact(got, og.render_all(osb, ofb, p.cs, 16))
        assert g.get_normalization_value("sum") == og.get_normalization_value("sum")
    g.reset_normalize_vertices()                                   # back to the running-peak form
    og.reset_normalize_vertices()
    got, fam = _profiled(g, lambda: g.render_all(sb, fb, p.cs, 16))
    assert ("k_scale" in fam) == fresh_two_pass and "k_norm_fix" not in fam
    assert_bit_exact(got, og.render_all(osb, ofb, p.cs, 16))


@pytest.mark.parametrize("bl,bits,chunk", [(1024, 16, 0), (333, 16, 0), (2048, 24, 0), (1024, 16, 7000), (64, 8, 0)])
def test_violated_speculation_falls_back_exactly(gpu_api, oracle, bl, bits, chunk):
    """The scan covers only the first blocks, the render the whole timeline: later blocks are louder than the carried
    max, the speculation fails in most tiles and k_norm_fix has to reproduce the running max block by block."""
    p = W.ProjectScript(48000, bl)
    p.set_length(1.5)
    p.set_render_bitdepth(bits)
    for k in range(5):
        p.assets["s%d" % k] = W.Asset(W.noise_int16(300 + k, 4001 + 313 * k))
        p.load_sample("s%d" % k, "s%d" % k, "")
        p.add_sampleloop("v%d" % k, 0.2 + 0.3 * k, -40.0 + 20.0 * k, "s%d" % k)
    p.add_normalize("inner", 0.8, 10.0)
    p.add_sum("mid", 1.3, 0.0)
    p.add_normalize("out", 1.0, -5.0)
    for k in range(5):
        p.connect("v%d" % k, "inner" if k < 3 else "mid")
    p.connect("inner", "mid")       # a Normalize feeding (through a Sum) another Normalize: both speculate
    p.connect("mid", "out")
    p.set_output("out")
    sb, fb, g = p.build(gpu_api)
    osb, ofb, og = p.build(oracle)
    if chunk:
        g.set_option("max_chunk_frames", chunk)
    g.true_normalize_scan(sb, fb, 2)
    og.true_normalize_scan(osb, ofb, 2)
    for rep in range(3):   # the first render fails the speculation and raises the carried max; later ones mostly keep it
        got, fam = _profiled(g, lambda: g.render_all(sb, fb, p.cs, bits))
        assert "k_norm_fix" in fam and "k_scale" not in fam
        assert_bit_exact(got, og.render_all(osb, ofb, p.cs, bits))
        for name in ("inner", "out"):
            assert g.get_normalization_value(name) == og.get_normalization_value(name)


def test_render_twice_after_scan_on_the_drum_project(gpu_api, oracle):
    """Carried vertex state (quirk Q4: sample_multi voices, lerp offsets, ADSR clocks survive set_time) makes the second
    render after a scan differ from what the scan saw."""
    p = W.drum_project(seconds=2.0)
    gb, ob = p.build(gpu_api), p.build(oracle)
    gb[2].true_normalize_scan(gb[0], gb[1], p.cs)
    ob[2].true_normalize_scan(ob[0], ob[1], p.cs)
    for _ in range(3):
        assert_bit_exact(p.render(gpu_api, built=gb), p.render(oracle, built=ob))
        assert gb[2].get_normalization_value("sum") == ob[2].get_normalization_value("sum")


def test_scanned_block_pulls_and_synth(gpu_api, oracle):
    p = W.synth_project(seconds=1.0)
    gb, ob = p.build(gpu_api), p.build(oracle)
    gb[2].true_normalize_scan(gb[0], gb[1], 5)      # short scan -> the render violates it
    ob[2].true_normalize_scan(ob[0], ob[1], 5)
    assert_close(p.render(gpu_api, built=gb), p.render(oracle, built=ob))
    q = W.drum_project(seconds=0.2)
    gsb, gfb, gg = q.build(gpu_api)
    osb, ofb, og = q.build(oracle)
    gg.true_normalize_scan(gsb, gfb, 3)
    og.true_normalize_scan(osb, ofb, 3)
    for b in range(q.cs):                           # one-block chunks through the speculative form
        gl, gr = gg.render(gsb, gfb)
        ol, orr = og.render(osb, ofb)
        assert np.array_equal(gl.view(np.uint32), ol.view(np.uint32)) and np.array_equal(gr.view(np.uint32), orr.view(np.uint32)), b
        gfb.set_time_to_next_block()
        ofb.set_time_to_next_block()


@pytest.mark.parametrize("project", ["config1", "config2_short", "config2_edge", "drum", "chain", "nested"])
@pytest.mark.parametrize("single", [1, 0])
def test_fresh_single_pass_normalize_is_value_identical(gpu_api, oracle, project, single):
    """Fresh (un-scanned) renders: the running-peak Normalize in one launch (option single_pass_normalize, default) against
    the two passes and the oracle, bit for bit -- packed-loop, f32 edge-buffer, Adsr-through and nested-Normalize inputs,
    rendered twice (the carried max moves on) and in chunks."""
    if project == "config1":
        p = W.config1(seconds=2.0)
    elif project in ("config2_short", "config2_edge"):
        p = W.config2(seconds=3.0, n_src=9)
    elif project == "drum":
        p = W.drum_project(seconds=2.0)
    elif project == "chain":
        p = W.config4(seconds=1.5, depth=6)
    else:
        p = W.ProjectScript(48000, 1024)
        p.set_length(2.0)
        for k in range(4):
            p.assets["s%d" % k] = W.Asset(W.noise_int16(500 + k, 3001 + 517 * k))
            p.load_sample("s%d" % k, "s%d" % k, "")
            p.add_sampleloop("v%d" % k, 0.3 + 0.2 * k, -30.0 + 20.0 * k, "s%d" % k)
        p.add_normalize("inner", 0.9, 5.0)
        p.add_normalize("out", 1.0, 0.0)
        for k in range(4):
            p.connect("v%d" % k, "inner" if k < 2 else "out")
        p.connect("inner", "out")
        p.set_output("out")
    gb, ob = p.build(gpu_api), p.build(oracle)
    gb[2].set_option("debug.single_pass_normalize", single)
    if project == "config2_edge":
        gb[2].set_option("fuse_sources", 0)
    for rep in range(2):
        assert_bit_exact(p.render(gpu_api, built=gb), p.render(oracle, built=ob))
    gb[2].set_option("max_chunk_frames", 9000)
    assert_bit_exact(p.render(gpu_api, built=gb), p.render(oracle, built=ob))
