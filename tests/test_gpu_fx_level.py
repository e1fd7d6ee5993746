"""All seven effect kinds in ONE level: a drum bus feeds a compressor, an EQ, a delay, a saturator, a chorus, a reverb and a gate in
parallel, the seven feed a Sum `mix`, and every effect vertex is a stem (graph B).  The per-kind suites put one kind in a level at a
time; here the kinds' lowerings share the level's scratch edge buffers, its scratch region and the loop over the launch families.

Against B stand seven graphs A, one per kind: the bus feeds that kind alone and the kind is the output.  Same kernels on the same
input, so everything is compared bitwise: a kind's frames in B are those of its own graph A.  The engine has no read-out of a stem's
f32 frames, so they are taken as the output's: B is rendered once per kind with that kind named as the output, the stem list -- and
with it the level of seven -- unchanged; the render with `mix` as the output compares the stems' PCM words.

0.25 s at 48 kHz in blocks of 256: about 12 k frames, longer than the 4 096 frames up to which the saturator and the chorus take their
one-launch forms (k_sat_sum / k_chorus_sum first) and six 2 048-frame tiles of the scans; in chunks of 4 096 frames neither *_sum
launch may appear.  The parameters are the per-kind suites' mid-range ones at wet 1, gain 1, angle 0; the delay's D = 1 024 keeps it
to one k_delay_apply tile in both forms, as in tests/test_gpu_fx_lines.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chorus_projects as CP  # noqa: E402
import eq_projects as EP  # noqa: E402
import test_gpu_eq as TG  # noqa: E402

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
}
LONG_FORM_ONLY = {"k_sat_sum", "k_chorus_sum"}   # (chunks of more than 4 096 frames)


def project(kinds, mix):
    p = EP.base_project("drums", bl=BL, seconds=0.25)
    for k in kinds:
        call, params = KINDS[k][:2]
        getattr(p, call)(k, 1.0, 0.0, 1.0, *params)
        p.connect("bus", k)
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


@pytest.fixture(scope="module")
def graphs(gpu_api):
    """B and the seven A, each after the discarded first render of tests/test_gpu_eq.py's build()."""
    pb = project(list(KINDS), mix=True)
    b = TG.build(gpu_api, pb)
    b[2].set_stems(list(KINDS))
    assert 5 * 2048 < pb.cs * BL <= 16 * 1024 and gpu_api.delay_params(48000, *KINDS["dly"][1])[0] == 1024
    a = {k: TG.build(gpu_api, project([k], mix=False)) for k in KINDS}
    return pb.cs, b, a


def profiled(g, render_):
    """render_() with profiling on: what it returns and the names of the launches it took."""
    g.set_profiling(1)
    y = render_()
    names = set(g.kernel_times())
    g.set_profiling(0)
    return y, names


def check_level(names, chunk, who):
    """The launches of ALL seven kinds are in `names`: the level held every kind, whichever vertex was the output."""
    for k, (_, _, launches, _) in KINDS.items():
        for n in launches:
            assert (n in names) == (chunk > 4096 or n not in LONG_FORM_ONLY), (who, k, n, sorted(names))
    assert "k_delay_local" not in names and "k_stems" in names, (who, sorted(names))


@pytest.mark.parametrize("chunk", [1 << 24, 4096])
def test_every_kind_in_one_level_has_the_bits_of_the_kind_alone(graphs, chunk):
    cs, b, a = graphs
    g = b[2]
    (mix_pcm, mix_f32), names = profiled(g, lambda: render(b, "mix", cs, chunk))
    check_level(names, chunk, "mix")
    stems = [g.read_stem_pcm(i) for i in range(len(KINDS))]
    assert np.isfinite(mix_f32).all() and np.abs(mix_f32).max() > 0.05
    for i, (k, (_, _, _, passes)) in enumerate(KINDS.items()):
        want_pcm, want = render(a[k], k, cs, chunk)
        assert np.isfinite(want).all() and np.abs(want).max() > (0.05 if passes else 0.0), k
        assert np.array_equal(stems[i], want_pcm), (k, "stem pcm", np.argwhere(stems[i] != want_pcm)[:4].tolist())
        # the kind as B's output: the stems keep the other six in its level (their launches are there), `mix` is not computed
        (_, got), k_names = profiled(g, lambda: render(b, k, cs, chunk))
        check_level(k_names, chunk, k)
        assert same_bits(got, want), (k, "f32", np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:4].tolist())
