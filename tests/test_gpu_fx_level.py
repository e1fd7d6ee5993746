"""The effect kinds in ONE level: a drum bus feeds the first n of a compressor, an EQ, a delay, a saturator, a chorus, a reverb, a
gate, a phaser, a vocoder, a filter, a limiter and a multiband in parallel, the n feed a Sum `mix`, and every effect vertex is a
stem (graph B); n = 7 .. 12, the sizes the level had as the kinds were added.  The vocoder and the filter take their key from the
snare alone, a vertex two levels up.  The per-kind suites put one kind in a level at a time; here the kinds' lowerings share the level's scratch
edge buffers, its scratch region and the loop over the launch families.

Against B stand graphs A, one per kind: the bus feeds that kind alone and the kind is the output.  Same kernels on the same input,
so everything is compared bitwise: a kind's frames in B are those of its own graph A.  The render with `mix` as the output compares
the stems' PCM words.  The engine has no read-out of a stem's f32 frames, so they are taken as the output's: B is rendered with the
kind named as the output, the stem list -- and with it the level of n -- unchanged; at n = 7 every kind is, above that the newest.

0.25 s at 48 kHz in blocks of 256: about 12 k frames, longer than the 4 096 frames up to which the saturator and the chorus take their
one-launch forms (k_sat_sum / k_chorus_sum first) and six 2 048-frame tiles of the scans; in chunks of 4 096 frames neither *_sum
launch may appear, the scans keep their launches at two tiles.  The limiter's lowering takes two scratch edge buffers and a carried
line beside the other kinds' in the same level; its window of 480 frames makes the chunks' second tile read its halo from the first
and the first from the line.  The multiband's takes four scratch edge buffers, a carried line, a block table in the arena and -- over
three descriptors of its own per vertex -- the compressor's k_comp_env and the scalar carry beside the compressor's own launches of
them in the same level.  The parameters are the per-kind suites' mid-range ones at wet 1,
gain 1, angle 0; the delay's D = 1 024 keeps it to one k_delay_apply tile in both forms, as in tests/test_gpu_fx_lines.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chorus_projects as CP  # noqa: E402
import eq_projects as EP  # noqa: E402
import fx_rig as TG  # noqa: E402

pytestmark = pytest.mark.gpu
BL = 256
# name -> (the ProjectScript call, its parameters behind (gain, angle, wet), the launches of a whole render, passes the dry signal on)
KINDS = {
    "comp": ("add_compressor", (-26.0, 4.0, 5.0, 400.0, 6.0, 2.0),
             ("k_comp_detect", "k_comp_carry_y1", "k_comp_env", "k_comp_carry_yl", "k_comp_apply"), True),
    "eq": ("add_eq", ("lowshelf", 120.0, 0.9, 9.0), ("k_eq_local", "k_eq_carry", "k_eq_apply"), True),
    "dly": ("add_delay", (1024.0 / 48.0, 0.7, 0.35), ("k_delay_apply",), True),
    "sat": ("add_saturator", ("soft", 12.0, 0.2, -3.0, 4), ("k_sat_sum", "k_sat"), True),
    "cho": ("add_chorus", CP.case(3, (20.0, 4.0, 0.8, 0.25), "sine"), ("k_chorus_sum", "k_chorus"), False),
    "rev": ("add_reverb", (0.5, 0.5, 0.5, 0.5), ("k_reverb_sum", "k_reverb"), False),
    "gate": ("add_gate", (-30.0, 6.0, 10.0, 1.0, 100.0, -20.0),
             ("k_gate_detect", "k_gate_carry_hc", "k_gate_env", "k_gate_carry_env", "k_gate_apply"), True),
    "pha": ("add_phaser", (6, 200.0, 2000.0, 1.0, 0.7, 0.25, "sine"), ("k_phaser_local", "k_phaser_carry", "k_phaser_apply"), True),
    "voc": ("add_vocoder", (16, 100.0, 8000.0, 6.0, 5.0, 24.0),
            ("k_voc_local", "k_voc_carry_z", "k_voc_env", "k_voc_carry_env", "k_voc_apply"), True),
    "filt": ("add_filter", ("lowpass", 400.0, 4.0, 2.0, 3.0, 0.25, "sine", 4.0, 18.0, 2.0, 80.0),
             ("k_filt_detect", "k_filt_carry_y1", "k_filt_env", "k_filt_carry_e", "k_filt_local", "k_filt_carry", "k_filt_apply"), True),
    "lim": ("add_limiter", (-6.0, 10.0, 50.0, 12.0), ("k_lim_detect", "k_lim_carry", "k_lim_apply"), True),
    "mb": ("add_multiband", (200.0, 2000.0, (-40.0, -30.0, -36.0), (4.0, 8.0, 2.0), 5.0, 50.0, 6.0, (0.0, 3.0, 6.0)),
           ("k_mb_local", "k_mb_carry", "k_mb_detect", "k_mb_carry_y1", "k_mb_env", "k_mb_carry_yl", "k_mb_apply"), True),
}
KEYED = ("voc", "filt")
LONG_FORM_ONLY = {"k_sat_sum", "k_chorus_sum"}   # (chunks of more than 4 096 frames)


def project(kinds, mix):
    p = EP.base_project("drums", bl=BL, seconds=0.25)
    for k in kinds:
        call, params = KINDS[k][:2]
        getattr(p, call)(k, 1.0, 0.0, 1.0, *params)
        p.connect("bus", k)
        if k in KEYED:
            p.connect_key("snare", k)
    if mix:
        p.add_sum("mix", 1.0, 0.0)
        for k in kinds:
            p.connect(k, "mix")
    p.set_output("mix" if mix else kinds[0])
    return p


def render(built, out, cs, chunk):
    """One whole-timeline render from time 0 with `out` as the output: (pcm, f32)."""
    sb, fb, g = built
    g.set_option("max_chunk_frames", chunk)
    assert g.set_output(out)
    fb.set_time(0)
    g.set_time(0)
    g.reset_normalize_vertices()
    return g.render_all(sb, fb, cs, 16)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def level(gpu_api, n):
    """(cs, B): the first n kinds in one level, every one a stem, after the discarded first render of tests/fx_rig.py's build()."""
    kinds = list(KINDS)[:n]
    pb = project(kinds, mix=True)
    b = TG.build(gpu_api, pb)
    b[2].set_stems(kinds)
    assert len(kinds) == n and 5 * 2048 < pb.cs * BL <= 16 * 1024
    return pb.cs, b


@pytest.fixture(scope="module")
def alone(gpu_api):
    """The twelve A, built like B: a kind alone computes the same whatever else B holds, so every level size shares them."""
    assert len(KINDS) == 12 and list(KINDS)[-2:] == ["lim", "mb"] and gpu_api.delay_params(48000, *KINDS["dly"][1])[0] == 1024
    assert gpu_api.limiter_params(48000, *KINDS["lim"][1])[2] == 480
    return {k: TG.build(gpu_api, project([k], mix=False)) for k in KINDS}


@pytest.fixture(scope="module", params=[7, 8, 9, 10, 11, 12])
def graphs(request, gpu_api, alone):
    """B of the first n kinds and their A."""
    cs, b = level(gpu_api, request.param)
    return cs, b, {k: alone[k] for k in list(KINDS)[:request.param]}


def profiled(g, render_):
    """render_() with profiling on: what it returns and the names of the launches it took."""
    g.set_profiling(1)
    y = render_()
    names = set(g.kernel_times())
    g.set_profiling(0)
    return y, names


def check_level(names, kinds, chunk, who):
    """The launches of ALL of `kinds` are in `names`: the level held every kind, whichever vertex was the output."""
    for k in kinds:
        for n in KINDS[k][2]:
            assert (n in names) == (chunk > 4096 or n not in LONG_FORM_ONLY), (who, k, n, sorted(names))
    assert "k_stems" in names, (who, sorted(names))
    if len(kinds) == 7:   # (the delay's one tile: nothing else in a level of these seven would bring the launch in either)
        assert "k_delay_local" not in names, (who, sorted(names))


@pytest.mark.parametrize("chunk", [1 << 24, 4096])
def test_every_kind_in_one_level_has_the_bits_of_the_kind_alone(graphs, chunk):
    cs, b, a = graphs
    g = b[2]
    kinds = list(a)
    (mix_pcm, mix_f32), names = profiled(g, lambda: render(b, "mix", cs, chunk))
    check_level(names, kinds, chunk, "mix")
    stems = [g.read_stem_pcm(i) for i in range(len(kinds))]
    assert np.isfinite(mix_f32).all() and np.abs(mix_f32).max() > 0.05
    want_f32 = {}
    for i, k in enumerate(kinds):
        want_pcm, want = render(a[k], k, cs, chunk)
        # (the seven alone hold the vocoder to 0.05 as well -- it is not among them; its own level is a band-limited product)
        assert np.isfinite(want).all() and np.abs(want).max() > (0.05 if KINDS[k][3] and k != "voc" else 0.0), k
        assert np.array_equal(stems[i], want_pcm), (k, "stem pcm", np.argwhere(stems[i] != want_pcm)[:4].tolist())
        want_f32[k] = want
    if "voc" in kinds:
        assert np.abs(want_f32["voc"]).max() > 0.005
    if "lim" in kinds:   # the limiter works on this bus: its stem is held under the ceiling, which the bus driven by 12 dB would pass
        assert np.abs(want_f32["lim"]).max() <= 10.0 ** (-6.0 / 20.0) * (1.0 + 2.0 ** -22)
    if "mb" in kinds:    # the multiband works on this bus: its stem differs from the bus by far more than a rounding
        bus = render(a["mb"], "bus", cs, chunk)[1]
        assert np.abs(want_f32["mb"].astype(np.float64) - bus).max() > 1e-2 * np.abs(bus).max()
    # a kind as B's output: the stems keep the others in its level (their launches are there), `mix` is not computed
    for k in (kinds if len(kinds) == 7 else kinds[-1:]):
        (_, got), k_names = profiled(g, lambda: render(b, k, cs, chunk))
        check_level(k_names, kinds, chunk, k)
        assert same_bits(got, want_f32[k]), (k, "f32", np.argwhere(got.view(np.uint32) != want_f32[k].view(np.uint32))[:4].tolist())


@pytest.mark.parametrize("chunk", [1 << 24, 4096])
def test_a_vertex_added_behind_set_time_leaves_every_kind_starting_afresh(gpu_api, chunk):
    """A state slot allocated while every effect vertex has a set_time pending and the device holds the end of a render: the
    host mirror is fetched, the kinds' states at time 0 are put back into it, and the next render has the bits of the first."""
    cs, b = level(gpu_api, len(KINDS))
    sb, fb, g = b
    render(b, "mix", cs, chunk)
    first = [g.read_stem_pcm(i) for i in range(len(KINDS))]
    assert all(np.abs(s).max() > 0 for s in first)
    fb.set_time(0)
    g.set_time(0)
    g.reset_normalize_vertices()
    g.add_normalize("late", 1.0, 0.0)   # (unconnected: a slot, and nothing else)
    g.render_all(sb, fb, cs, 16)
    for i, k in enumerate(KINDS):
        again = g.read_stem_pcm(i)
        assert np.array_equal(again, first[i]), (k, "stem pcm", np.argwhere(again != first[i])[:4].tolist())
