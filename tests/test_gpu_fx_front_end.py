"""Both front ends, all thirteen effect kinds, against the words of the commit tests/golden/fx_front_end.json was recorded on.

The project is tests/test_gpu_fx_level13.py's: the drum bus into the twelve kinds of tests/test_gpu_fx_level.py and a
convolution vertex (tests/test_gpu_convolution.py's smallest case, a response of two frames from a load_sample asset) in parallel,
the thirteen into a Sum `mix`; 0.25 s at 48 kHz in blocks of 256.  Thirteen kinds in one level put every kind's parameters
through its lowering at once; 12 k frames is over the 4 096-frame one-launch forms and six 2 048-frame scan tiles.

It is rendered twice from a fresh engine: built by ProjectScript.build (the C entry points td_graph_add_*) and by api.State from
to_lua() (the script line's binder and the replay), under the same engine options.  The two front ends add the multiband and the
convolution vertex in opposite orders, which moves vertex indices and must not reach a sample."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_projects as CP  # noqa: E402
import fx_rig as TG  # noqa: E402
import test_gpu_convolution as GC  # noqa: E402
import test_gpu_fx_level as L  # noqa: E402

pytestmark = pytest.mark.gpu
OPTIONS = {"sine_mode": 1, "band_mode": 0}   # (the exact forms, on both paths: their defaults differ)


def project():
    p = L.project(list(L.KINDS), mix=False)
    name = GC.CASE2[0]
    CP.load_response(p, name, CP.response_int16(int(name[1:]), 0))
    p.add_convolution("cv", 1.0, 0.0, 1.0, *GC.CASE2)
    p.connect("bus", "cv")
    p.add_sum("mix", 1.0, 0.0)
    for k in list(L.KINDS) + ["cv"]:
        p.connect(k, "mix")
    p.set_output("mix")
    return p


def digest(pcm):
    return hashlib.sha256(np.ascontiguousarray(pcm, dtype="<i2").tobytes()).hexdigest()


def renders(api, tmp_dir):
    """(the int16 words by the C entry points, by the script)."""
    p = project()
    assert len(p.calls["add_convolution"]) == 1 and sum(len(p.calls[L.KINDS[k][0]]) for k in L.KINDS) == 12
    sb, fb, g = p.build(api)
    for k, v in OPTIONS.items():
        g.set_option(k, v)
    abi = g.render_all(sb, fb, p.cs, 16, want_f32=False)[0]
    d = os.path.join(str(tmp_dir), "proj")
    TG._write_project(p, d)
    st = api.State(open_dir=d)
    for k, v in OPTIONS.items():
        st.set_option(k, v)
    assert st.refresh(), api.last_error()
    return abi, st.render_to_memory()


def test_both_front_ends_render_the_recorded_words(gpu_api, tmp_path):
    want = json.load(open(os.path.join(TG.TESTS, "golden", "fx_front_end.json")))["render"]
    abi, script = renders(gpu_api, tmp_path)
    assert abi.shape == script.shape == (want["frames"], 2) and np.abs(abi).max() > 1000
    assert np.array_equal(abi, script), np.argwhere(abi != script)[:4].tolist()
    assert digest(abi) == want["abi_sha256"] and digest(script) == want["script_sha256"]
