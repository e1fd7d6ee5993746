"""The convolution vertex on the device (td_graph_add_convolution) against its float64 twin (tests/np_convolution.py,
the definition in include/termdaw_amd.h as a direct sum), run on the engine's own constants (td_convolution_params) and on the
response as the bank holds it (SampleBank.get_sample).

The input of the vertex under test always comes from the engine itself: a second render of the same graph with set_output on
the vertex in front, read as f32 -- the oracle-verified part of the graph is not restated here.

Bounds.  wet = 1, gain = 1, angle = 0, per value:  |p' - p| <= 2^-23 |p| + E max|p| on the convolved signal p, carried through the
definition's f32 lerp to the vertex' output (fx_rig.assert_close says why it is not asserted on the output as it stands).  The
first term is the one f32 rounding of the chain, which may flip; E covers the float64 roundings of the transforms and of the sum
over the partitions: 8 x what the numpy emulation of the kernels' arithmetic shows against a long-double direct sum over this
file's own grid and inputs (tests/conv_projects.py E, derived and re-checked on the CPU by tests/test_convolution_host.py; under
the cap 2^-28).  With wet in (0, 1), pan and gain: 4 x 2^-23 x max(|dry|, |p|) x |amplitude| absolute, as for the EQ.

Every case prints its worst error over the bound."""
import os
import sys

import numpy as np
import pytest

from termdaw_amd import workloads as W

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_projects as CP  # noqa: E402
import fx_rig  # noqa: E402
import np_convolution as NC  # noqa: E402
from fx_rig import MIX, _pull_all, assert_close, build, render_f32  # noqa: E402

pytestmark = pytest.mark.gpu
CONV_LAUNCHES = ["k_conv_fwd", "k_conv_mac", "k_conv_inv"]
FIRST_LAUNCHES = ["k_conv_ir"] + CONV_LAUNCHES               # the render that builds the vertex' spectra: its first
# Two partitions, normalised.  No pre-delay in the placement tests: the transforms' error is absolute, E max|p|, so where the
# definition's p is exactly 0 -- in front of a pre-delayed response -- the device's is some 1e-17, and a second vertex behind it
# would be measured on that stretch by the rig's mix bound, which is relative to the value alone (the grid and the chunk tests
# below hold every pre-delay to the bound that has the absolute term).
CASE = ("h1025", 0.0, 0.0, -6.0, 1)
CASE2 = ("h2", 0.0, 0.0, 0.0, 0)
_responses = {}


def base_project(kind, **kw):
    """conv_projects' base project with the grid's responses loaded: a case names one of them."""
    p = CP.base_project(kind, **kw)
    CP.load_grid_responses(p)
    return p


def response(api, sr, name):
    """The response `name` as the bank holds it at rate sr: float32 [Lh, 2] (read once per process)."""
    if (sr, name) not in _responses:
        p = W.ProjectScript(sr, 1024)
        pcm = CP.sparse_int16() if name == "sparse" else CP.response_int16(int(name[1:]), 0)
        CP.load_response(p, name, pcm)
        sb = api.SampleBank(sr)
        a = p.assets[name]
        sb.add_decoded(name, a.pcm.astype(np.float32).reshape(-1), a.channels, a.sr, a.bits, "")
        l, r = sb.get_sample(sb.get_index(name))
        _responses[(sr, name)] = np.stack([l, r], axis=1).astype(np.float32)
    return _responses[(sr, name)]


def consts(api, sr, case):
    """(h as used, D, g with norm applied) of a case."""
    name, length_ms, predelay_ms, out_db, norm = case
    h = response(api, sr, name)
    Lh, D, g, P, H, Bp = api.convolution_params(sr, len(h), length_ms, predelay_ms, out_db, norm)
    assert Bp == NC.B
    h = h[:Lh]
    return h, D, NC.scale(h, g, norm)


def twin(api, sr, case, x, state=None):
    h, D, g = consts(api, sr, case)
    return NC.direct(x, h, D, g, state)


def mix(api, sr, case, x, **kw):
    h, D, g = consts(api, sr, case)
    return NC.process(x, h, D, g, **kw)[0]


def close(y, xd, p, what):
    return assert_close(y, xd, p, what, CP.E)


CONV = fx_rig.FxKind("convolution", "k_conv", FIRST_LAUNCHES, CP.add_convolution, base_project, CASE, CASE2, CP.E,
                     twin=lambda api, sr, case, x: twin(api, sr, case, x)[:2], mix=mix)


def _conv_launches(g):
    return [n for n in g.kernel_times() if n.startswith("k_conv")]


# ---- the grid ----
@pytest.mark.parametrize("sr", CP.RATES)
@pytest.mark.parametrize("kind", CP.INPUTS)
def test_grid_matches_the_twin(gpu_api, sr, kind):
    cases = CP.grid_cases(sr)
    assert len(cases) == 48
    p = base_project(kind, sr=sr)
    for i, (c, _, _) in enumerate(cases):
        CP.add_convolution(p, "c%d" % i, "bus", c)
    built = build(gpu_api, p)
    x = render_f32(gpu_api, built, "bus", p.cs)
    n = p.cs * p.bl
    assert np.abs(x).max() > 0.05 and n > 5 * NC.B
    worst, exact = 0.0, 0
    core = {}   # per response: the convolution itself, shared by its six cases (pre-delay and trim are a shift and a factor)
    for i, (c, Lh, D) in enumerate(cases):
        k = gpu_api.convolution_params(sr, Lh, *c[1:])
        assert k[0] == Lh and k[1] == D and k[3] == -(-(D + Lh) // NC.B) and k[4] == D + Lh - 1
        h, D2, g = consts(gpu_api, sr, c)
        assert D2 == D and len(h) == Lh and np.abs(h[:, 0] - h[:, 1]).max() > 0.1
        if Lh not in core:
            core[Lh] = NC.direct64(x, h, 0, 1.0)[0]
        p64 = np.zeros_like(core[Lh])
        p64[D:] = g * core[Lh][:n - D]
        pw = p64.astype(np.float32)
        assert np.abs(pw).max() > 1e-3
        y = render_f32(gpu_api, built, "c%d" % i, p.cs)
        worst = max(worst, close(y, x, pw, "%s %d %s" % (kind, sr, c)))
        want = x + np.float32(1.0) * (pw - x)
        exact += int(np.array_equal(y.view(np.uint32), want.view(np.uint32)))
    print("grid %s %d: %d cases, worst |y - want| %.3g x the plain bound, %d bit-identical to the twin" % (kind, sr, len(cases), worst, exact))
    assert np.array_equal(render_f32(gpu_api, built, "bus", p.cs), x)   # (and every render above saw this input)


@pytest.mark.parametrize("sr", CP.RATES)
def test_sparse_response_at_the_cap(gpu_api, sr):
    """262 144 frames of response, five taps, 6 s of drums: 256 partitions, and the last tap sounds."""
    p = CP.base_project("drums", sr=sr, seconds=CP.SPARSE_SECONDS)
    CP.load_response(p, "sparse", CP.sparse_int16())
    case = ("sparse", 0.0, 0.0, -6.0, 0)
    CP.add_convolution(p, "c", "bus", case)
    built = build(gpu_api, p)
    x = render_f32(gpu_api, built, "bus", p.cs)
    h, D, g = consts(gpu_api, sr, case)
    assert len(h) == CP.CAP and D == 0 and gpu_api.convolution_params(sr, CP.CAP, 0.0, 0.0, -6.0, 0)[3] == 256
    taps = [(k, h[k]) for k in CP.SPARSE_TAPS]
    assert np.count_nonzero(h) == 2 * len(taps)
    p64 = NC.sparse64(x, taps, D, g)
    n = len(x)
    assert n > CP.CAP and np.abs(x[:n - CP.CAP + 1]).max() > 0.05   # (the last tap sounds)
    y = render_f32(gpu_api, built, "c", p.cs)
    close(y, x, p64.astype(np.float32), "sparse %d" % sr)


# ---- chunks, pulls, restarts ----
@pytest.mark.parametrize("chunk", [63, 1023, 1024, 1025, 2049, 4097])
def test_chunked_renders_match_the_unchunked_twin(gpu_api, chunk):
    """Chunks of `chunk` frames (block length = chunk, one block per chunk) against the twin in one piece: every alignment of tile
    and chunk, the carried frames crossing every cut."""
    seconds = 0.1 if chunk == 63 else 0.5
    p = base_project("noise", bl=chunk, seconds=seconds)
    case = ("h2049", 0.0, CP.predelay_ms(48000, 1), -6.0, 0)
    CP.add_convolution(p, "c", "bus", case)
    built = build(gpu_api, p)
    x = render_f32(gpu_api, built, "bus", p.cs)
    pw, xd, _ = twin(gpu_api, 48000, case, x)
    y = [render_f32(gpu_api, built, "c", p.cs, max_chunk_frames=chunk) for _ in range(2)]
    assert p.cs > 5
    close(y[0], xd, pw, "chunks of %d" % chunk)
    assert np.array_equal(y[0].view(np.uint32), y[1].view(np.uint32))   # a second render after set_time(0) is bitwise the first
    built[2].set_option("max_chunk_frames", 1 << 24)
    whole = render_f32(gpu_api, built, "c", p.cs)
    close(whole, xd, pw, "whole, bl %d" % chunk)
    # the state really crosses the cuts: restarted from silence, chunk 3 would be far outside the bound
    restart = twin(gpu_api, 48000, case, x[3 * chunk:4 * chunk])[0]
    assert np.abs(restart.astype(np.float64) - pw[3 * chunk:4 * chunk]).max() > 1e-3


@pytest.mark.parametrize("bl", [64, 1024])
def test_block_pulls_match_the_twin_and_set_time_empties_the_history(gpu_api, bl):
    p = base_project("noise", bl=bl, seconds=0.1 if bl == 64 else 0.5)
    case = ("h1025", 0.0, CP.predelay_ms(48000, 1), -6.0, 1)   # (1 025 carried frames: sixteen pulls of 64 deep)
    CP.add_convolution(p, "c", "bus", case)
    built = build(gpu_api, p)
    x = render_f32(gpu_api, built, "bus", p.cs)
    pw, xd, _ = twin(gpu_api, 48000, case, x)
    pulls = [_pull_all(gpu_api, built, "c", p.cs) for _ in range(2)]
    close(pulls[0], xd, pw, "pulls of %d" % bl)
    assert np.array_equal(pulls[0].view(np.uint32), pulls[1].view(np.uint32))
    # a set_time in the middle of pulling restarts the vertex from silence: two pulls, a jump, one pull
    at = (4000 // bl) * bl
    got = []
    for out in ("c", "bus"):
        sb, fb, g = p.build(gpu_api)
        assert g.set_output(out)
        for _ in range(2):
            g.render(sb, fb)
            fb.set_time_to_next_block()
        fb.set_time(at)
        g.set_time(at)
        got.append(np.stack(g.render(sb, fb), axis=1))
    assert np.abs(got[1]).max() > 0.01
    after = twin(gpu_api, 48000, case, got[1])[0]
    assert np.abs(after).max() > 1e-3
    close(got[0], got[1], after, "pull after set_time")
    assert np.abs(after.astype(np.float64) - pw[at:at + bl]).max() > 1e-3   # (the running render has the history there)


# ---- the mix ----
@pytest.mark.parametrize("wet,gain,angle", MIX)
def test_wet_pan_and_gain(gpu_api, wet, gain, angle):
    fx_rig.wet_pan_and_gain(gpu_api, CONV, wet, gain, angle, vertex="c")


def test_dry_passes_the_input_through(gpu_api):
    fx_rig.dry_passes_the_input_through(gpu_api, CONV)


# ---- placement ----
def test_in_front_of_a_normalize_output(gpu_api):
    fx_rig.in_front_of_a_normalize_output(gpu_api, CONV, vertex="c")


def test_as_a_stem_and_two_in_series(gpu_api):
    fx_rig.as_a_stem_and_two_in_series(gpu_api, CONV, "c1", "c2")


def test_fed_by_an_inlined_loop_source_and_a_gain_stage(gpu_api):
    # (the rig's project has no response of its own: the kind's add loads it)
    def add(p, name, src, case, **kw):
        if case[0] not in p.assets:
            CP.load_response(p, case[0], CP.response_int16(int(case[0][1:]), 0))
        CP.add_convolution(p, name, src, case, **kw)
    kind = CONV._replace(add=add)
    fx_rig.fed_by_an_inlined_loop_source_and_a_gain_stage(gpu_api, kind, CASE, W.noise_int16(50, 9000), vertex="c")


def test_batch_members_are_bitwise_their_own_renders(gpu_api):
    # three different partition counts: 1, 2 and 5 (h3073 with a pre-delay of one partition)
    cases = [("h1024", 0.0, 0.0, -6.0, 1), ("h1025", 0.0, 1.0, -12.0, 0), ("h3073", 0.0, CP.predelay_ms(48000, 1024), -6.0, 1)]
    assert sorted({gpu_api.convolution_params(48000, int(c[0][1:]), *c[1:])[3] for c in cases}) == [1, 2, 5]
    fx_rig.batch_members_are_bitwise_their_own_renders(gpu_api, CONV, CP.INPUTS, cases, vertex="cv")


def test_projects_without_a_convolution_launch_no_convolution_kernel(gpu_api):
    fx_rig.projects_without_the_kind_launch_no_kernel_of_it(gpu_api, "k_conv")
    sb, fb, g = fx_rig.a_whole_render_launches_the_kinds_kernels(gpu_api, CONV, vertex="c")
    # a block pull runs the same launches over one tile; the spectra stand
    g.set_time(0)
    fb.set_time(0)
    g.set_profiling(1)
    g.render(sb, fb)
    assert _conv_launches(g) == CONV_LAUNCHES


def test_spectra_are_built_once_per_response(gpu_api):
    """The first render of a vertex launches k_conv_ir in front of the three; a second render over the same bank does not; a bank
    whose sample was replaced launches it again, and the render is the new response's."""
    p = base_project("drums")
    CP.add_convolution(p, "c", "bus", CASE)
    p.set_output("c")
    sb, fb, g = p.build(gpu_api)
    g.set_profiling(1)
    g.render_all(sb, fb, p.cs, 16, want_f32=False)
    assert _conv_launches(g) == FIRST_LAUNCHES
    for _ in range(2):
        fb.set_time(0)
        g.set_time(0)
        g.set_profiling(1)
        first = g.render_all(sb, fb, p.cs, 16, want_pcm=False)[1]
        assert _conv_launches(g) == CONV_LAUNCHES
    # the same project over a bank that holds another sample under the name
    q = base_project("drums")
    q.assets["h1025"] = W.Asset(CP.response_int16(1025, 9), sr=q.psr)
    sb2 = q.build(gpu_api)[0]
    fb.set_time(0)
    g.set_time(0)
    g.set_profiling(1)
    second = g.render_all(sb2, fb, p.cs, 16, want_pcm=False)[1]
    assert _conv_launches(g) == FIRST_LAUNCHES
    assert np.abs(second - first).max() > 1e-3
    l, r = sb2.get_sample(sb2.get_index("h1025"))
    h = np.stack([l, r], axis=1).astype(np.float32)
    assert g.set_output("bus")
    fb.set_time(0)
    g.set_time(0)
    x = g.render_all(sb2, fb, p.cs, 16, want_pcm=False)[1]
    Lh, D, g0 = gpu_api.convolution_params(48000, 1025, *CASE[1:])[:3]
    pw = NC.direct(x, h, D, NC.scale(h, g0, 1))[0]
    close(second, x, pw, "replaced response")


def test_an_all_zero_response_with_norm_is_an_error_that_names_norm(gpu_api):
    p = CP.base_project("drums")
    CP.load_response(p, "z", np.zeros((100, 2), np.int16))
    CP.add_convolution(p, "c", "bus", ("z", 0.0, 0.0, 0.0, 1))
    p.set_output("c")
    sb, fb, g = p.build(gpu_api)
    with pytest.raises(gpu_api.TermdawError, match="norm"):
        g.render_all(sb, fb, p.cs, 16)


def test_a_response_over_the_cap_is_refused_by_name(gpu_api, tmp_path):
    """... where the bank is first seen: by the render, and by State.refresh; length_ms trims it into range."""
    p = CP.base_project("drums")
    CP.load_response(p, "long", np.ones((CP.CAP + 1, 2), np.int16))
    CP.add_convolution(p, "c", "bus", ("long", 0.0, 0.0, 0.0, 0))
    p.set_output("c")
    sb, fb, g = p.build(gpu_api)
    with pytest.raises(gpu_api.TermdawError, match="length_ms"):
        g.render_all(sb, fb, p.cs, 16)
    d = str(tmp_path / "proj")
    fx_rig._write_project(p, d)
    st = gpu_api.State(open_dir=d)
    assert not st.refresh()
    assert "length_ms" in gpu_api.last_error() and "262144" in gpu_api.last_error(), gpu_api.last_error()
    p.calls["add_convolution"][0] = ("c", 1.0, 0.0, 1.0, "long", 1000.0, 0.0, 0.0, 0)
    i = [j for j, (fn, _) in enumerate(p.script_order) if fn == "add_convolution"][0]
    p.script_order[i] = ("add_convolution", p.calls["add_convolution"][0])
    fx_rig._write_project(p, d)
    st = gpu_api.State(open_dir=d)
    assert st.refresh(), gpu_api.last_error()


# ---- the guard modes ----
def _guard_project(conv_first):
    p = fx_rig.gpu_guard_base()
    CP.load_response(p, "h1025", CP.response_int16(1025, 0))
    p.add_convolution("c", 1.0, 0.0, 1.0, *CASE)
    if conv_first:   # loop -> vertex -> band-pass chain; the synth joins behind the vertex
        p.connect("s", "c"); p.connect("c", "b1"); p.connect("b1", "b2"); p.connect("b2", "bus"); p.connect("y", "bus")
        p.set_output("bus")
    else:            # band-pass chain and synth -> bus -> vertex
        p.connect("s", "b1"); p.connect("b1", "b2"); p.connect("b2", "bus"); p.connect("y", "bus"); p.connect("bus", "c")
        p.set_output("c")
    return p


def test_guard_keeps_the_scan_and_fast_sines_downstream_of_a_convolution(gpu_api):
    fx_rig.guard_keeps_the_scan_and_fast_sines_downstream(gpu_api, _guard_project(True), "convolution", "k_conv", FIRST_LAUNCHES)


def test_guard_renders_the_exact_forms_upstream_of_a_convolution(gpu_api):
    fx_rig.guard_renders_the_exact_forms_upstream(gpu_api, _guard_project(False))


# ---- the front end ----
def test_front_end_renders_a_convolved_drum_bus(gpu_api, tmp_path):
    mem = fx_rig.front_end_renders(gpu_api, tmp_path, W.convolution_project(seconds=1.0), 'add_convolution("conv",')
    fx_rig.front_end_words_differ(gpu_api, tmp_path, W.convolution_project(seconds=1.0, wet=0.0), mem)
