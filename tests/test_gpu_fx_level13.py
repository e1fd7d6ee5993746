"""All thirteen effect kinds in ONE level, in the form of tests/test_gpu_fx_level.py (whose table, projects and checks this file
takes over): the drum bus feeds the twelve kinds of that file and a convolution vertex in parallel, the thirteen feed a Sum `mix`,
every effect vertex is a stem (graph B).  Against B stand graphs A, one per kind, the kind alone as the output; same kernels on
the same input, so everything is compared bitwise.

The convolution's lowering takes one scratch edge buffer, a carried line, a spectra block of its own and -- per chunk -- some
64 bytes per frame of the submission's scratch region beside the other kinds' tile words; its response of 1 025 frames behind a
pre-delay of 48 makes two partitions, so every tile reads two window spectra, the chunks' first tiles from the line."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_projects as CP  # noqa: E402
import eq_projects as EP  # noqa: E402
import fx_rig as TG  # noqa: E402
import test_gpu_fx_level as L  # noqa: E402

pytestmark = pytest.mark.gpu
CONV = ("add_convolution", ("h1025", 0.0, 1.0, -6.0, 1), ("k_conv_fwd", "k_conv_mac", "k_conv_inv"), True)
KINDS = dict(L.KINDS, cv=CONV)


def project(kinds, mix):
    if "cv" not in kinds:
        return L.project(kinds, mix)
    others = [k for k in kinds if k != "cv"]
    p = L.project(others, mix=False) if others else EP.base_project("drums", bl=L.BL, seconds=0.25)
    CP.load_response(p, "h1025", CP.response_int16(1025, 0))
    p.add_convolution("cv", 1.0, 0.0, 1.0, *CONV[1])
    p.connect("bus", "cv")
    if mix:
        p.add_sum("mix", 1.0, 0.0)
        for k in kinds:
            p.connect(k, "mix")
    p.set_output("mix" if mix else kinds[0])
    return p


@pytest.fixture(scope="module")
def graphs(gpu_api):
    kinds = list(KINDS)
    assert len(kinds) == 13 and kinds[-1] == "cv" and gpu_api.convolution_params(48000, 1025, *CONV[1][1:])[3] == 2
    pb = project(kinds, mix=True)
    b = TG.build(gpu_api, pb)
    b[2].set_stems(kinds)
    assert 5 * 2048 < pb.cs * L.BL <= 16 * 1024
    alone = {k: TG.build(gpu_api, project([k], mix=False)) for k in kinds}
    return pb.cs, b, alone


def check_level(names, chunk, who):
    for k, spec in KINDS.items():
        for n in spec[2]:
            assert (n in names) == (chunk > 4096 or n not in L.LONG_FORM_ONLY), (who, k, n, sorted(names))
    assert "k_stems" in names, (who, sorted(names))


@pytest.mark.parametrize("chunk", [1 << 24, 4096])
def test_thirteen_kinds_in_one_level_have_the_bits_of_each_kind_alone(graphs, chunk):
    cs, b, a = graphs
    g = b[2]
    kinds = list(KINDS)
    (mix_pcm, mix_f32), names = L.profiled(g, lambda: L.render(b, "mix", cs, chunk))
    check_level(names, chunk, "mix")
    stems = [g.read_stem_pcm(i) for i in range(len(kinds))]
    assert np.isfinite(mix_f32).all() and np.abs(mix_f32).max() > 0.05
    want_f32 = {}
    for i, k in enumerate(kinds):
        want_pcm, want = L.render(a[k], k, cs, chunk)
        assert np.isfinite(want).all(), k
        assert np.array_equal(stems[i], want_pcm), (k, "stem pcm", np.argwhere(stems[i] != want_pcm)[:4].tolist())
        want_f32[k] = want
    # the convolution works on this bus: its stem differs from the bus by far more than a rounding
    bus = L.render(a["cv"], "bus", cs, chunk)[1]
    assert np.abs(want_f32["cv"].astype(np.float64) - bus).max() > 1e-2 * np.abs(bus).max()
    # the newest kind as B's output: the stems keep the others in its level, `mix` is not computed
    (_, got), k_names = L.profiled(g, lambda: L.render(b, "cv", cs, chunk))
    check_level(k_names, chunk, "cv")
    assert L.same_bits(got, want_f32["cv"]), np.argwhere(got.view(np.uint32) != want_f32["cv"].view(np.uint32))[:4].tolist()
