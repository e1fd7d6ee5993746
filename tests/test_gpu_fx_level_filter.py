"""All TEN effect kinds in one level, in the manner of tests/test_gpu_fx_level_vocoder.py (which stays as it is, with its nine): a
drum bus feeds a compressor, an EQ, a delay, a saturator, a chorus, a reverb, a gate, a phaser, a vocoder and a filter in
parallel, the ten feed a Sum `mix`, and every effect vertex is a stem (graph B).  The vocoder and the filter take their key from
the snare alone, a vertex two levels up.  The filter's lowering shares the level's scratch edge buffers (two of them: x and the
level words), its scratch region and the loop over the launch families with the other nine.

Against B stands graph A: the bus feeds the filter alone and the filter is the output.  Same kernels on the same input, so the
comparison is bitwise: the filter's stem in B holds the PCM words of A, and B rendered with the filter named as the output (the
stem list -- and with it the level of ten -- unchanged) holds A's f32 frames.  The other nine are held to their own graphs A the
same way: the tenth kind in their level changes none of their bits.

0.25 s at 48 kHz in blocks of 256: about 12 k frames, six 2 048-frame tiles of the filter's scans (seven launches); in chunks of
4 096 frames two tiles, the same seven launches."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eq_projects as EP  # noqa: E402
import test_gpu_eq as TG  # noqa: E402
import test_gpu_fx_level as FL  # noqa: E402
import test_gpu_fx_level_vocoder as FV  # noqa: E402

pytestmark = pytest.mark.gpu
BL = FL.BL
KEYED = ("voc", "filt")
KINDS = dict(FV.KINDS)
KINDS["filt"] = ("add_filter", ("lowpass", 400.0, 4.0, 2.0, 3.0, 0.25, "sine", 4.0, 18.0, 2.0, 80.0),
                 ("k_filt_detect", "k_filt_carry_y1", "k_filt_env", "k_filt_carry_e", "k_filt_local", "k_filt_carry", "k_filt_apply"), True)


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
    """B and the ten A, each after the discarded first render of tests/test_gpu_eq.py's build()."""
    pb = project(list(KINDS), mix=True)
    b = TG.build(gpu_api, pb)
    b[2].set_stems(list(KINDS))
    assert len(KINDS) == 10 and 5 * 2048 < pb.cs * BL <= 16 * 1024
    a = {k: TG.build(gpu_api, project([k], mix=False)) for k in KINDS}
    return pb.cs, b, a


def check_level(names, chunk, who):
    """The launches of ALL ten kinds are in `names`: the level held every kind, whichever vertex was the output."""
    for k, (_, _, launches, _) in KINDS.items():
        for n in launches:
            assert (n in names) == (chunk > 4096 or n not in FL.LONG_FORM_ONLY), (who, k, n, sorted(names))
    assert "k_stems" in names, (who, sorted(names))


@pytest.mark.parametrize("chunk", [1 << 24, 4096])
def test_every_kind_in_one_level_of_ten_has_the_bits_of_the_kind_alone(graphs, chunk):
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
    # the filter as B's output: the stems keep the other nine in its level (their launches are there), `mix` is not computed
    want = FL.render(a["filt"], "filt", cs, chunk)[1]
    (_, got), k_names = FL.profiled(g, lambda: FL.render(b, "filt", cs, chunk))
    check_level(k_names, chunk, "filt")
    assert FL.same_bits(got, want), ("filt", "f32", np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:4].tolist())
