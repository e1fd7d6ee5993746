"""All EIGHT effect kinds in one level, in the manner of tests/test_gpu_fx_level.py (which stays as it is, with its seven): a drum
bus feeds a compressor, an EQ, a delay, a saturator, a chorus, a reverb, a gate and a phaser in parallel, the eight feed a Sum
`mix`, and every effect vertex is a stem (graph B).  The phaser's lowering shares the level's scratch edge buffers, its scratch
region and the loop over the launch families with the other seven.

Against B stands graph A: the bus feeds the phaser alone and the phaser is the output.  Same kernels on the same input, so the
comparison is bitwise: the phaser's stem in B holds the PCM words of A, and B rendered with the phaser named as the output (the
stem list -- and with it the level of eight -- unchanged) holds A's f32 frames.  The other seven are held to their own graphs A the
same way: the eighth kind in their level changes none of their bits.

0.25 s at 48 kHz in blocks of 256: about 12 k frames, six 2 048-frame tiles of the phaser's scan (k_phaser_local, k_phaser_carry,
k_phaser_apply); in chunks of 4 096 frames two tiles, the same three launches."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eq_projects as EP  # noqa: E402
import test_gpu_eq as TG  # noqa: E402
import test_gpu_fx_level as FL  # noqa: E402

pytestmark = pytest.mark.gpu
BL = FL.BL
KINDS = dict(FL.KINDS)
KINDS["pha"] = ("add_phaser", (6, 200.0, 2000.0, 1.0, 0.7, 0.25, "sine"), ("k_phaser_local", "k_phaser_carry", "k_phaser_apply"), True)


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


@pytest.fixture(scope="module")
def graphs(gpu_api):
    """B and the eight A, each after the discarded first render of tests/test_gpu_eq.py's build()."""
    pb = project(list(KINDS), mix=True)
    b = TG.build(gpu_api, pb)
    b[2].set_stems(list(KINDS))
    assert len(KINDS) == 8 and 5 * 2048 < pb.cs * BL <= 16 * 1024
    a = {k: TG.build(gpu_api, project([k], mix=False)) for k in KINDS}
    return pb.cs, b, a


def check_level(names, chunk, who):
    """The launches of ALL eight kinds are in `names`: the level held every kind, whichever vertex was the output."""
    for k, (_, _, launches, _) in KINDS.items():
        for n in launches:
            assert (n in names) == (chunk > 4096 or n not in FL.LONG_FORM_ONLY), (who, k, n, sorted(names))
    assert "k_stems" in names, (who, sorted(names))


@pytest.mark.parametrize("chunk", [1 << 24, 4096])
def test_every_kind_in_one_level_of_eight_has_the_bits_of_the_kind_alone(graphs, chunk):
    cs, b, a = graphs
    g = b[2]
    (mix_pcm, mix_f32), names = FL.profiled(g, lambda: FL.render(b, "mix", cs, chunk))
    check_level(names, chunk, "mix")
    stems = [g.read_stem_pcm(i) for i in range(len(KINDS))]
    assert np.isfinite(mix_f32).all() and np.abs(mix_f32).max() > 0.05
    for i, (k, (_, _, _, passes)) in enumerate(KINDS.items()):
        want_pcm, want = FL.render(a[k], k, cs, chunk)
        assert np.isfinite(want).all() and np.abs(want).max() > (0.05 if passes else 0.0), k
        assert np.array_equal(stems[i], want_pcm), (k, "stem pcm", np.argwhere(stems[i] != want_pcm)[:4].tolist())
    # the phaser as B's output: the stems keep the other seven in its level (their launches are there), `mix` is not computed
    want = FL.render(a["pha"], "pha", cs, chunk)[1]
    (_, got), k_names = FL.profiled(g, lambda: FL.render(b, "pha", cs, chunk))
    check_level(k_names, chunk, "pha")
    assert FL.same_bits(got, want), ("pha", "f32", np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:4].tolist())
