"""All twelve effect kinds in ONE level: tests/test_gpu_fx_level11.py's graphs with the multiband as the twelfth kind.  A drum bus
feeds a compressor, an EQ, a delay, a saturator, a chorus, a reverb, a gate, a phaser, a vocoder, a filter, a limiter and a
multiband in parallel, the twelve feed a Sum `mix`, and every effect vertex is a stem (graph B).  Against B stand graphs A, one per
kind: the bus feeds that kind alone and the kind is the output.  Same kernels on the same input, so everything is compared bitwise:
a kind's frames in B are those of its own graph A, whole and in chunks of 4 096 frames.  The multiband's lowering takes four scratch
edge buffers, a carried line, a block table in the arena and -- over three descriptors of its own per vertex -- the compressor's
k_comp_env and the scalar carry beside the compressor's own launches of them in the same level."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eq_projects as EP  # noqa: E402
import test_gpu_eq as TG  # noqa: E402
from test_gpu_fx_level import BL, KEYED, LONG_FORM_ONLY, profiled, render, same_bits  # noqa: E402
from test_gpu_fx_level11 import KINDS as KINDS11  # noqa: E402

pytestmark = pytest.mark.gpu
KINDS = dict(KINDS11)
KINDS["mb"] = ("add_multiband", (200.0, 2000.0, (-40.0, -30.0, -36.0), (4.0, 8.0, 2.0), 5.0, 50.0, 6.0, (0.0, 3.0, 6.0)),
               ("k_mb_local", "k_mb_carry", "k_mb_detect", "k_mb_carry_y1", "k_mb_env", "k_mb_carry_yl", "k_mb_apply"), True)


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
    """(cs, B, the twelve A), each after the discarded first render of tests/test_gpu_eq.py's build()."""
    assert len(KINDS) == 12 and list(KINDS)[-1] == "mb"
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
    # the multiband works on this bus: its stem differs from the bus by far more than a rounding
    bus = render(a["mb"], "bus", cs, chunk)[1]
    assert np.abs(want_f32["mb"].astype(np.float64) - bus).max() > 1e-2 * np.abs(bus).max()
    # the newest kind as B's output: the stems keep the others in its level (their launches are there), `mix` is not computed
    (_, got), k_names = profiled(g, lambda: render(b, "mb", cs, chunk))
    check_level(k_names, chunk, "mb")
    assert same_bits(got, want_f32["mb"]), ("mb", "f32", np.argwhere(got.view(np.uint32) != want_f32["mb"].view(np.uint32))[:4].tolist())
