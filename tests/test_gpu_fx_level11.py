"""All eleven effect kinds in ONE level: tests/test_gpu_fx_level.py's graphs with the limiter as the eleventh kind.  A drum bus
feeds a compressor, an EQ, a delay, a saturator, a chorus, a reverb, a gate, a phaser, a vocoder, a filter and a limiter in
parallel, the eleven feed a Sum `mix`, and every effect vertex is a stem (graph B).  Against B stand graphs A, one per kind: the
bus feeds that kind alone and the kind is the output.  Same kernels on the same input, so everything is compared bitwise: a
kind's frames in B are those of its own graph A, whole and in chunks of 4 096 frames.  The limiter's lowering takes two scratch
edge buffers and a carried line beside the other kinds' in the same level; its window of 480 frames makes the chunks' second tile
read its halo from the first and the first from the line."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eq_projects as EP  # noqa: E402
import test_gpu_eq as TG  # noqa: E402
from test_gpu_fx_level import BL, KEYED, KINDS as KINDS10, LONG_FORM_ONLY, profiled, render, same_bits  # noqa: E402

pytestmark = pytest.mark.gpu
KINDS = dict(KINDS10)
KINDS["lim"] = ("add_limiter", (-6.0, 10.0, 50.0, 12.0), ("k_lim_detect", "k_lim_carry", "k_lim_apply"), True)


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


@pytest.fixture(scope="module")
def graphs(gpu_api):
    """(cs, B, the eleven A), each after the discarded first render of tests/test_gpu_eq.py's build()."""
    assert len(KINDS) == 11 and list(KINDS)[-1] == "lim" and gpu_api.limiter_params(48000, *KINDS["lim"][1])[2] == 480
    kinds = list(KINDS)
    pb = project(kinds, mix=True)
    b = TG.build(gpu_api, pb)
    b[2].set_stems(kinds)
    assert 5 * 2048 < pb.cs * BL <= 16 * 1024
    return pb.cs, b, {k: TG.build(gpu_api, project([k], mix=False)) for k in kinds}


def check_level(names, chunk, who):
    """The launches of ALL the kinds are in `names`: the level held every kind, whichever vertex was the output."""
    for k in KINDS:
        for n in KINDS[k][2]:
            assert (n in names) == (chunk > 4096 or n not in LONG_FORM_ONLY), (who, k, n, sorted(names))
    assert "k_stems" in names, (who, sorted(names))


@pytest.mark.parametrize("chunk", [1 << 24, 4096])
def test_every_kind_in_one_level_has_the_bits_of_the_kind_alone(graphs, chunk):
    cs, b, a = graphs
    g = b[2]
    kinds = list(KINDS)
    (mix_pcm, mix_f32), names = profiled(g, lambda: render(b, "mix", cs, chunk))
    check_level(names, chunk, "mix")
    stems = [g.read_stem_pcm(i) for i in range(len(kinds))]
    assert np.isfinite(mix_f32).all() and np.abs(mix_f32).max() > 0.05
    want_f32 = {}
    for i, k in enumerate(kinds):
        want_pcm, want = render(a[k], k, cs, chunk)
        assert np.isfinite(want).all() and np.abs(want).max() > (0.05 if KINDS[k][3] and k != "voc" else 0.0), k
        assert np.array_equal(stems[i], want_pcm), (k, "stem pcm", np.argwhere(stems[i] != want_pcm)[:4].tolist())
        want_f32[k] = want
    # the limiter works on this bus: its stem is held under the ceiling, which the bus driven by 12 dB would pass
    assert np.abs(want_f32["lim"]).max() <= 10.0 ** (-6.0 / 20.0) * (1.0 + 2.0 ** -22)
    # the newest kind as B's output: the stems keep the others in its level (their launches are there), `mix` is not computed
    (_, got), k_names = profiled(g, lambda: render(b, "lim", cs, chunk))
    check_level(k_names, chunk, "lim")
    assert same_bits(got, want_f32["lim"]), ("lim", "f32", np.argwhere(got.view(np.uint32) != want_f32["lim"].view(np.uint32))[:4].tolist())
