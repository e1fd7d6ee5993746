"""All NINE effect kinds in one level, in the manner of tests/test_gpu_fx_level_phaser.py (which stays as it is, with its eight): a
drum bus feeds a compressor, an EQ, a delay, a saturator, a chorus, a reverb, a gate, a phaser and a vocoder in parallel, the nine
feed a Sum `mix`, and every effect vertex is a stem (graph B).  The vocoder takes its key from the snare alone, a vertex two levels
up.  Its lowering shares the level's scratch edge buffers (two of them: x and the key sum), its scratch region and the loop over
the launch families with the other eight.

Against B stands graph A: the bus feeds the vocoder alone and the vocoder is the output.  Same kernels on the same input, so the
comparison is bitwise: the vocoder's stem in B holds the PCM words of A, and B rendered with the vocoder named as the output (the
stem list -- and with it the level of nine -- unchanged) holds A's f32 frames.  The other eight are held to their own graphs A the
same way: the ninth kind in their level changes none of their bits.

0.25 s at 48 kHz in blocks of 256: about 12 k frames, six 2 048-frame tiles of the vocoder's scans (five launches); in chunks of
4 096 frames two tiles, the same five launches."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eq_projects as EP  # noqa: E402
import test_gpu_eq as TG  # noqa: E402
import test_gpu_fx_level as FL  # noqa: E402
import test_gpu_fx_level_phaser as FP  # noqa: E402

pytestmark = pytest.mark.gpu
BL = FL.BL
KINDS = dict(FP.KINDS)
KINDS["voc"] = ("add_vocoder", (16, 100.0, 8000.0, 6.0, 5.0, 24.0), ("k_voc_local", "k_voc_carry_z", "k_voc_env", "k_voc_carry_env", "k_voc_apply"), True)


def project(kinds, mix):
    p = EP.base_project("drums", bl=BL, seconds=0.25)
    for k in kinds:
        call, params = KINDS[k][:2]
        getattr(p, call)(k, 1.0, 0.0, 1.0, *params)
        p.connect("bus", k)
        if k == "voc":
            p.connect_key("snare", "voc")
    if mix:
        p.add_sum("mix", 1.0, 0.0)
        for k in kinds:
            p.connect(k, "mix")
    p.set_output("mix" if mix else kinds[0])
    return p


@pytest.fixture(scope="module")
def graphs(gpu_api):
    """B and the nine A, each after the discarded first render of tests/test_gpu_eq.py's build()."""
    pb = project(list(KINDS), mix=True)
    b = TG.build(gpu_api, pb)
    b[2].set_stems(list(KINDS))
    assert len(KINDS) == 9 and 5 * 2048 < pb.cs * BL <= 16 * 1024
    a = {k: TG.build(gpu_api, project([k], mix=False)) for k in KINDS}
    return pb.cs, b, a


def check_level(names, chunk, who):
    """The launches of ALL nine kinds are in `names`: the level held every kind, whichever vertex was the output."""
    for k, (_, _, launches, _) in KINDS.items():
        for n in launches:
            assert (n in names) == (chunk > 4096 or n not in FL.LONG_FORM_ONLY), (who, k, n, sorted(names))
    assert "k_stems" in names, (who, sorted(names))


@pytest.mark.parametrize("chunk", [1 << 24, 4096])
def test_every_kind_in_one_level_of_nine_has_the_bits_of_the_kind_alone(graphs, chunk):
    cs, b, a = graphs
    g = b[2]
    (mix_pcm, mix_f32), names = FL.profiled(g, lambda: FL.render(b, "mix", cs, chunk))
    check_level(names, chunk, "mix")
    stems = [g.read_stem_pcm(i) for i in range(len(KINDS))]
    assert np.isfinite(mix_f32).all() and np.abs(mix_f32).max() > 0.05
    for i, (k, (_, _, _, passes)) in enumerate(KINDS.items()):
        want_pcm, want = FL.render(a[k], k, cs, chunk)
        assert np.isfinite(want).all() and np.abs(want).max() > (0.05 if passes and k != "voc" else 0.0), k
        assert np.array_equal(stems[i], want_pcm), (k, "stem pcm", np.argwhere(stems[i] != want_pcm)[:4].tolist())
    assert np.abs(FL.render(a["voc"], "voc", cs, chunk)[1]).max() > 0.005   # (the vocoder's own level: a band-limited product)
    # the vocoder as B's output: the stems keep the other eight in its level (their launches are there), `mix` is not computed
    want = FL.render(a["voc"], "voc", cs, chunk)[1]
    (_, got), k_names = FL.profiled(g, lambda: FL.render(b, "voc", cs, chunk))
    check_level(k_names, chunk, "voc")
    assert FL.same_bits(got, want), ("voc", "f32", np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:4].tolist())
