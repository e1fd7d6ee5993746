"""ctypes binding of the C ABI (include/termdaw_amd.h -> termdaw_amd/lib/libtermdaw_amd.so).

The classes keep the reference's names and method meanings (SampleBank sample.rs:187-348, FlowwBank
floww.rs:6-141, Graph graph.rs:12-238, State state.rs:27-578) so that parity tests read like tests of
the reference.  Everything renders on the GPU through the HIP library; there is no CPU fallback --
a missing library or missing device raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libtermdaw_amd.so")
_LIB_OVERRIDE = os.environ.get("TD_LIB")   # A/B experiments only (tools/ab_lib.py)


class TermdawError(RuntimeError):
    pass


class td_event(C.Structure):
    _fields_ = [("t_sec", C.c_float), ("note", C.c_float), ("vel", C.c_float)]


_lib = None

# name -> (restype, argtypes); also used by the symbol-export test
_f32, _sz, _vp, _cp, _i32, _lng = C.c_float, C.c_size_t, C.c_void_p, C.c_char_p, C.c_int, C.c_long
_fp = C.POINTER(C.c_float)
SIGNATURES = {
    "td_last_error": (_cp, []),
    "td_device_count": (_i32, []),
    "td_set_device": (_i32, [_i32]),
    "td_samplebank_new": (_vp, [_sz]),
    "td_samplebank_free": (None, [_vp]),
    "td_samplebank_add_file": (_i32, [_vp, _cp, _cp, _cp]),
    "td_samplebank_add_decoded": (_i32, [_vp, _cp, _fp, _sz, _i32, _sz, _sz, _cp]),
    "td_samplebank_get_index": (_lng, [_vp, _cp]),
    "td_samplebank_sample_len": (_sz, [_vp, _sz]),
    "td_samplebank_read": (_i32, [_vp, _sz, _fp, _fp]),
    "td_samplebank_get_max_sr_bd": (None, [_vp, C.POINTER(_sz), C.POINTER(_sz)]),
    "td_flowwbank_new": (_vp, [_sz, _sz]),
    "td_flowwbank_free": (None, [_vp]),
    "td_flowwbank_reset": (None, [_vp]),
    "td_flowwbank_add_events": (_lng, [_vp, _cp, C.POINTER(td_event), _sz]),
    "td_flowwbank_add_midi": (_lng, [_vp, _cp, _cp]),
    "td_flowwbank_declare_stream": (_lng, [_vp, _cp]),
    "td_flowwbank_append_stream": (_lng, [_vp, _cp, C.POINTER(td_event), _sz]),
    "td_flowwbank_trim_streams": (None, [_vp]),
    "td_flowwbank_get_events": (_sz, [_vp, _sz, C.POINTER(td_event), _sz]),
    "td_flowwbank_get_index": (_lng, [_vp, _cp]),
    "td_flowwbank_set_time": (None, [_vp, _sz]),
    "td_flowwbank_set_time_to_next_block": (None, [_vp]),
    "td_graph_new": (_vp, [_sz, _sz]),
    "td_graph_free": (None, [_vp]),
    "td_graph_reset": (None, [_vp]),
    "td_graph_add_sum": (_i32, [_vp, _cp, _f32, _f32]),
    "td_graph_add_normalize": (_i32, [_vp, _cp, _f32, _f32]),
    "td_graph_add_sampleloop": (_i32, [_vp, _cp, _f32, _f32, _sz]),
    "td_graph_add_sample_multi": (_i32, [_vp, _cp, _f32, _f32, _sz, _sz, _i32]),
    "td_graph_add_sample_lerp": (_i32, [_vp, _cp, _f32, _f32, _sz, _sz, _i32, _i32]),
    "td_graph_add_debug_sine": (_i32, [_vp, _cp, _f32, _f32, _sz]),
    "td_graph_add_synth": (_i32, [_vp, _cp, _f32, _f32, _sz, _f32, _f32, _fp, _i32, _f32, _f32, _fp, _i32, _f32, _fp, _i32]),
    "td_graph_add_adsr": (_i32, [_vp, _cp, _f32, _f32, _f32, _sz, _i32, _i32, _i32, _fp, _i32]),
    "td_graph_add_sampsyn": (_i32, [_vp, _cp, _f32, _f32, _sz, _fp, _i32, _cp, _sz]),
    "td_graph_add_bandpass": (_i32, [_vp, _cp, _f32, _f32, _f32, _f32, _f32, _i32]),
    "td_graph_add_compressor": (_i32, [_vp, _cp, _f32, _f32, _f32, _f32, _f32, _f32, _f32, _f32, _f32]),
    "td_graph_add_eq": (_i32, [_vp, _cp, _f32, _f32, _f32, _i32, _f32, _f32, _f32]),
    "td_eq_coefficients": (_i32, [_i32, _sz, _f32, _f32, _f32, C.POINTER(C.c_double)]),
    "td_graph_add_delay": (_i32, [_vp, _cp, _f32, _f32, _f32, _f32, _f32, _f32]),
    "td_delay_params": (_i32, [_sz, _f32, _f32, _f32, C.POINTER(C.c_double)]),
    "td_graph_add_saturator": (_i32, [_vp, _cp, _f32, _f32, _f32, _i32, _f32, _f32, _f32, _i32]),
    "td_saturator_taps": (_i32, [_i32, C.POINTER(C.c_double), _sz]),
    "td_saturator_params": (_i32, [_i32, _i32, _f32, _f32, _f32, C.POINTER(C.c_double)]),
    "td_graph_add_chorus": (_i32, [_vp, _cp, _f32, _f32, _f32, _i32, _f32, _f32, _f32, _f32, _i32]),
    "td_chorus_params": (_i32, [_sz, _i32, _f32, _f32, _f32, _f32, _i32, C.POINTER(C.c_double)]),
    "td_graph_add_reverb": (_i32, [_vp, _cp, _f32, _f32, _f32, _f32, _f32, _f32, _f32]),
    "td_graph_add_phaser": (_i32, [_vp, _cp, _f32, _f32, _f32, _i32, _f32, _f32, _f32, _f32, _f32, _i32]),
    "td_phaser_params": (_i32, [_sz, _i32, _f32, _f32, _f32, _f32, _f32, _i32, C.POINTER(C.c_double)]),
    "td_graph_add_gate": (_i32, [_vp, _cp, _f32, _f32, _f32, _f32, _f32, _f32, _f32, _f32, _f32]),
    "td_graph_add_vocoder": (_i32, [_vp, _cp, _f32, _f32, _f32, _i32, _f32, _f32, _f32, _f32, _f32]),
    "td_vocoder_params": (_i32, [_sz, _i32, _f32, _f32, _f32, _f32, _f32, C.POINTER(C.c_double), _sz]),
    "td_graph_add_filter": (_i32, [_vp, _cp, _f32, _f32, _f32, _i32, _f32, _f32, _f32, _f32, _f32, _i32, _f32, _f32, _f32, _f32]),
    "td_filter_params": (_i32, [_sz, _i32, _f32, _f32, _f32, _f32, _f32, _i32, _f32, _f32, _f32, _f32, C.POINTER(C.c_double), _sz]),
    "td_graph_add_limiter": (_i32, [_vp, _cp, _f32, _f32, _f32, _f32, _f32, _f32, _f32]),
    "td_limiter_params": (_i32, [_sz, _f32, _f32, _f32, _f32, C.POINTER(C.c_double)]),
    "td_graph_add_multiband": (_i32, [_vp, _cp, _f32, _f32, _f32, _f32, _f32, C.POINTER(C.c_float), C.POINTER(C.c_float), _f32, _f32, _f32, C.POINTER(C.c_float)]),
    "td_multiband_params": (_i32, [_sz, _f32, _f32, C.POINTER(C.c_float), C.POINTER(C.c_float), _f32, _f32, _f32, C.POINTER(C.c_float), C.POINTER(C.c_double), _sz]),
    "td_graph_add_convolution": (_i32, [_vp, _cp, _f32, _f32, _f32, _sz, _f32, _f32, _f32, _i32]),
    "td_convolution_params": (_i32, [_sz, _sz, _f32, _f32, _f32, _i32, C.POINTER(C.c_double)]),
    "td_convolution_twiddles": (_sz, [C.POINTER(C.c_double), _sz]),
    "td_gate_params": (_i32, [_sz, _f32, _f32, _f32, _f32, _f32, _f32, C.POINTER(C.c_double)]),
    "td_reverb_params": (_i32, [_sz, _f32, _f32, _f32, _f32, C.POINTER(C.c_double)]),
    "td_graph_connect": (_i32, [_vp, _cp, _cp]),
    "td_graph_connect_key": (_i32, [_vp, _cp, _cp]),
    "td_graph_set_output": (_i32, [_vp, _cp]),
    "td_graph_check": (_i32, [_vp]),
    "td_graph_set_time": (None, [_vp, _sz]),
    "td_graph_change_time": (_sz, [_vp, _sz, _i32]),
    "td_graph_get_time": (_sz, [_vp]),
    "td_graph_reset_normalize_vertices": (None, [_vp]),
    "td_graph_get_normalization_value": (_f32, [_vp, _cp]),
    "td_graph_vertex_count": (_sz, [_vp]),
    "td_graph_render_block": (_i32, [_vp, _vp, _vp, _fp, _fp]),
    "td_graph_normalize_scan": (_i32, [_vp, _vp, _vp, _sz]),
    "td_graph_render_all": (_sz, [_vp, _vp, _vp, _sz, _i32]),
    "td_graph_render_all_resampled": (_sz, [_vp, _vp, _vp, _sz, _i32, _sz, _sz]),
    "td_graph_output_pcm_device": (_vp, [_vp]),
    "td_graph_output_f32_device": (_vp, [_vp]),
    "td_graph_read_pcm": (_i32, [_vp, _vp, _sz]),
    "td_graph_read_f32": (_i32, [_vp, _fp, _sz]),
    "td_graph_output_peak": (_f32, [_vp]),
    "td_graph_set_stems": (_i32, [_vp, C.POINTER(_cp), _sz]),
    "td_graph_stem_count": (_sz, [_vp]),
    "td_graph_stem_pcm_device": (_vp, [_vp, _sz]),
    "td_graph_read_stem_pcm": (_i32, [_vp, _sz, _vp, _sz]),
    "td_graph_stem_peak": (_f32, [_vp, _sz]),
    "td_graph_loudness": (_i32, [_vp, C.POINTER(C.c_double), _sz]),
    "td_graph_momentary": (_sz, [_vp, _sz, C.POINTER(C.c_double), _sz]),
    "td_loudness_f32": (_i32, [_fp, _sz, _sz, C.POINTER(C.c_double)]),
    "td_loudness_filters": (_i32, [_sz, C.POINTER(C.c_double), _fp, _sz, C.POINTER(_sz), C.POINTER(_sz)]),
    "td_graph_master": (_i32, [_vp, C.c_double, C.c_double, C.c_double, C.c_double, C.POINTER(C.c_double)]),
    "td_master_f32": (_i32, [_fp, _sz, _sz, C.c_double, C.c_double, C.c_double, C.c_double, _fp, C.POINTER(C.c_double)]),
    "td_graph_render_all_async": (_sz, [_vp, _vp, _vp, _sz, _i32]),
    "td_graph_sync": (_i32, [_vp]),
    "td_graph_norm_fix_runs": (_sz, [_vp]),
    "td_graph_norm_respec": (_sz, [_vp]),
    "td_graph_set_profiling": (None, [_vp, _i32]),
    "td_graph_host_times": (_sz, [_vp, C.POINTER(C.c_double), _i32]),
    "td_graph_last_kernel_times": (_sz, [_vp, C.POINTER(_cp), _fp, C.POINTER(_sz), _sz]),
    "td_graph_device_bytes": (_sz, [_vp]),
    "td_trim_memory": (None, []),
    "td_device_sinf": (_i32, [_fp, _fp, _sz, _i32]),
    "td_cached_memory_bytes": (_sz, []),
    "td_graph_set_option": (_i32, [_vp, _cp, _lng]),
    "td_graph_get_option": (_i32, [_vp, _cp, C.POINTER(_lng)]),
    "td_graph_option_key": (_cp, [_sz]),
    "td_graph_band_stats": (_i32, [_vp, C.POINTER(C.c_uint32)]),
    "td_graph_band_guard_stats": (_i32, [_vp, C.POINTER(C.c_double)]),
    "td_batch_new": (_vp, []),
    "td_batch_free": (None, [_vp]),
    "td_batch_add": (_lng, [_vp, _vp, _vp, _vp]),
    "td_batch_size": (_sz, [_vp]),
    "td_batch_rewind": (None, [_vp]),
    "td_batch_render_all": (_sz, [_vp, _sz, _i32]),
    "td_batch_render_all_async": (_sz, [_vp, _sz, _i32]),
    "td_batch_sync": (_i32, [_vp]),
    "td_batch_normalize_scan": (_i32, [_vp, _sz]),
    "td_batch_render_to_files": (_i32, [_vp, _sz, _i32, _sz, C.POINTER(_cp), _i32, _i32, C.POINTER(C.c_double)]),
    "td_batch_host_pcm": (_vp, [_vp, _sz, C.POINTER(_sz)]),
    "td_batch_peaks": (_i32, [_vp, _fp]),
    "td_batch_peak_table_device": (_i32, [_vp, _vp, _sz, _sz, _sz]),
    "td_batch_loudness": (_i32, [_vp, C.POINTER(C.c_double)]),
    "td_batch_master": (_i32, [_vp, C.c_double, C.c_double, C.c_double, C.c_double, C.POINTER(C.c_double)]),
    "td_comm_unique_id": (_i32, [_vp, _sz]),
    "td_comm_init": (_vp, [_vp, _sz, _i32, _i32]),
    "td_comm_init_host": (_vp, [_vp, _vp, _i32, _i32]),
    "td_comm_free": (None, [_vp]),
    "td_comm_backend": (_cp, [_vp]),
    "td_comm_library": (_cp, []),
    "td_batch_exchange_peaks": (_i32, [_vp, _vp, _sz]),
    "td_batch_peak_table": (_vp, [_vp, C.POINTER(_sz)]),
    "td_batch_read_peak_table": (_i32, [_vp, _fp, _sz]),
    "td_batch_set_profiling": (None, [_vp, _i32]),
    "td_batch_last_kernel_times": (_sz, [_vp, C.POINTER(_cp), _fp, C.POINTER(_sz), _sz]),
    "td_batch_host_times": (_sz, [_vp, C.POINTER(C.c_double), _i32]),
    "td_batch_mark": (_i32, [_vp, _i32]),
    "td_batch_marked_ms": (C.c_double, [_vp]),
    "td_state_new": (_vp, [_cp, _sz, _sz]),
    "td_state_open": (_vp, [_cp]),
    "td_state_free": (None, [_vp]),
    "td_state_set_option": (_i32, [_vp, _cp, _lng]),
    "td_state_refresh_source": (_i32, [_vp, _cp]),
    "td_state_refresh": (_i32, [_vp]),
    "td_state_scan_exact": (_i32, [_vp]),
    "td_state_render": (_i32, [_vp, _cp]),
    "td_state_set_stems": (_i32, [_vp, C.POINTER(_cp), _sz]),
    "td_state_set_master": (_i32, [_vp, _i32, C.c_double, C.c_double]),
    "td_state_master_report": (_i32, [_vp, C.POINTER(C.c_double)]),
    "td_state_render_to_memory": (_sz, [_vp, _vp, _sz]),
    "td_state_render_view": (_vp, [_vp, C.POINTER(_sz)]),
    "td_state_chunk_count": (_sz, [_vp]),
    "td_state_render_samplerate": (_sz, [_vp]),
    "td_state_bitdepth": (_sz, [_vp]),
    "td_state_output_file": (_cp, [_vp]),
    "td_state_buffer_length": (_sz, [_vp]),
    "td_state_project_samplerate": (_sz, [_vp]),
    "td_state_graph": (_vp, [_vp]),
    "td_state_samplebank": (_vp, [_vp]),
    "td_state_flowwbank": (_vp, [_vp]),
    "td_state_dump_calls": (_cp, [_vp]),
}


def build(force=False):
    """hipcc build of the in-tree HIP library (termdaw_amd/Makefile); rebuilds when a source is newer."""
    import glob
    import subprocess
    srcs = glob.glob(os.path.join(_HERE, "csrc", "*")) + [os.path.join(_HERE, "..", "include", "termdaw_amd.h"),
                                                         os.path.join(_HERE, "Makefile")]
    def stale():
        return (not os.path.exists(LIB_PATH)) or any(os.path.getmtime(s) > os.path.getmtime(LIB_PATH)
                                                     for s in srcs if os.path.exists(s))
    if force or stale():
        # one builder at a time: the ranks of a multi-GPU launch all come through here at once
        import fcntl
        with open(os.path.join(_HERE, ".build.lock"), "w") as lk:
            fcntl.flock(lk, fcntl.LOCK_EX)
            try:
                if force or stale():
                    subprocess.check_call(["make", "-C", _HERE, "-j8", "-s"])
            finally:
                fcntl.flock(lk, fcntl.LOCK_UN)
    return LIB_PATH


def lib():
    """Loads the HIP library, building it first if the in-tree .so is missing or older than its sources.
    There is no CPU fallback: if hipcc cannot build it, this raises."""
    global _lib
    if _lib is None:
        # A stale or missing library whose rebuild fails is an error: tests and bench must never run a binary
        # that is older than the sources they claim to measure.  Only an explicit opt-in skips the build:
        # TD_LIB=<path> (A/B experiments) or TD_NO_BUILD=1 (a box without hipcc, prebuilt .so shipped along).
        if not (_LIB_OVERRIDE or os.environ.get("TD_NO_BUILD") == "1"):
            try:
                build()
            except Exception as e:   # noqa: BLE001
                raise TermdawError("`make -C termdaw_amd` failed (%s) and %s is missing or older than its sources; "
                                   "there is no CPU fallback (TD_NO_BUILD=1 loads a prebuilt library as it is)"
                                   % (e, LIB_PATH))
        if not os.path.exists(_LIB_OVERRIDE or LIB_PATH):
            raise TermdawError("%s is missing; there is no CPU fallback" % (_LIB_OVERRIDE or LIB_PATH))
        L = C.CDLL(_LIB_OVERRIDE or LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            if _LIB_OVERRIDE and name == "td_graph_norm_respec" and not hasattr(L, name):
                continue   # (A/B runs against a library built before the counter existed)
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def last_error():
    return lib().td_last_error().decode(errors="replace")


def _check(ok):
    if not ok:
        raise TermdawError(last_error())
    return ok


def _fa(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a, a.ctypes.data_as(_fp)


def _names(names):
    names = [n.encode() for n in names]
    return (_cp * max(1, len(names)))(*names), len(names)


# -- loudness (ITU-R BS.1770-4 / EBU Tech 3341 / 3342; include/termdaw_amd.h td_graph_loudness) --
LOUDNESS_FIELDS = ("integrated", "momentary_max", "short_term_max", "lra", "true_peak", "sample_peak", "frames", "sr")


def _loudness_dicts(out, n):
    rows = []
    for i in range(n):
        v = [float(x) for x in out[8 * i:8 * i + 8]]
        d = dict(zip(LOUDNESS_FIELDS, v))
        d["frames"], d["sr"] = int(v[6]), int(v[7])
        rows.append(d)
    return rows


def loudness_f32(frames, sr):
    """The meter over host frames: a (N, 2) float32 array (L, R) at rate sr, measured on the device -> one dict of
    LOUDNESS_FIELDS (integrated / momentary_max / short_term_max in LUFS, lra in LU, true_peak in dBTP, sample_peak in dBFS)."""
    a = np.ascontiguousarray(frames, dtype=np.float32).reshape(-1, 2)
    out = (C.c_double * 8)()
    _check(lib().td_loudness_f32(a.ctypes.data_as(_fp), a.shape[0], int(sr), out))
    return _loudness_dicts(out, 1)[0]


EQ_KINDS = ("lowpass", "highpass", "bandpass", "notch", "peak", "lowshelf", "highshelf")   # TD_EQ_* 0 .. 6, the Lua line's names


def eq_kind(kind):
    """A kind name of EQ_KINDS (or an index) as the TD_EQ_* integer."""
    if isinstance(kind, str):
        if kind not in EQ_KINDS:
            raise ValueError("eq: unknown kind %r (one of %s)" % (kind, ", ".join(EQ_KINDS)))
        return EQ_KINDS.index(kind)
    return int(kind)


def eq_coefficients(kind, sr, freq_hz, q, gain_db):
    """The EQ vertex' filter at rate sr (host only): (b, a) as float64 arrays with a[0] = 1, exactly as the engine uses them,
    and Hmax, the largest |H(e^jw)|."""
    out = (C.c_double * 6)()
    _check(lib().td_eq_coefficients(eq_kind(kind), int(sr), freq_hz, q, gain_db, out))
    k = np.array(out[:], np.float64)
    return k[0:3].copy(), np.array([1.0, k[3], k[4]]), float(k[5])


def delay_params(sr, time_ms, feedback, cross):
    """The delay vertex' constants at rate sr (host only), exactly as the engine uses them: (D, gs, gc, Hecho) -- the delay in
    frames, the straight and the crossed feedback gain, and 1 / (1 - feedback), the L2 gain of the echo path."""
    out = (C.c_double * 4)()
    _check(lib().td_delay_params(int(sr), time_ms, feedback, cross, out))
    return int(out[0]), float(out[1]), float(out[2]), float(out[3])


SAT_KINDS = ("hard", "cubic", "soft")   # TD_SAT_* in order


def sat_kind(kind):
    """A kind name of SAT_KINDS (or an index) as the TD_SAT_* integer."""
    if isinstance(kind, str):
        if kind not in SAT_KINDS:
            raise ValueError("saturator kind %r: one of %s" % (kind, ", ".join(SAT_KINDS)))
        return SAT_KINDS.index(kind)
    return int(kind)


def saturator_taps(oversample):
    """The saturator vertex' prototype low-pass at oversampling factor R (host only): the engine's own 2 * 32 * R + 1 taps as
    a float64 array."""
    n = lib().td_saturator_taps(int(oversample), None, 0)
    _check(n)
    out = (C.c_double * n)()
    _check(lib().td_saturator_taps(int(oversample), out, n))
    return np.array(out[:], np.float64)


def saturator_params(kind, oversample, drive_db, bias, out_db):
    """The saturator vertex' constants (host only), exactly as the engine uses them: (g_in, g_out, f(bias), latency in frames,
    Lf, Hsat) -- Hsat the gain the guard carries its estimate through the wet path at."""
    out = (C.c_double * 6)()
    _check(lib().td_saturator_params(sat_kind(kind), int(oversample), drive_db, bias, out_db, out))
    return float(out[0]), float(out[1]), float(out[2]), int(out[3]), float(out[4]), float(out[5])


CHORUS_SHAPES = ("sine", "triangle")   # TD_CHORUS_* in order


def chorus_shape(shape):
    """A shape name of CHORUS_SHAPES (or an index) as the TD_CHORUS_* integer."""
    if isinstance(shape, str):
        if shape not in CHORUS_SHAPES:
            raise ValueError("chorus shape %r: one of %s" % (shape, ", ".join(CHORUS_SHAPES)))
        return CHORUS_SHAPES.index(shape)
    return int(shape)


def phaser_params(sr, stages, lo_hz, hi_hz, rate_hz, feedback, stereo, shape):
    """(N, a_lo, a_hi, am, ad, f, fb): the phaser vertex' constants at rate sr, exactly the doubles the engine uses (host only; N an
    int).  shape: the chorus' names."""
    out = (C.c_double * 7)()
    _check(lib().td_phaser_params(int(sr), int(stages), lo_hz, hi_hz, rate_hz, feedback, stereo, chorus_shape(shape), out))
    return (int(out[0]),) + tuple(out[1:7])


FILTER_KINDS = ("lowpass", "highpass", "bandpass", "notch")   # TD_FILTER_* in order


def filter_kind(kind):
    """A kind name of FILTER_KINDS (or an index) as the TD_FILTER_* integer."""
    if isinstance(kind, str):
        if kind not in FILTER_KINDS:
            raise ValueError("filter kind %r: one of %s" % (kind, ", ".join(FILTER_KINDS)))
        return FILTER_KINDS.index(kind)
    return int(kind)


def filter_params(sr, kind, freq_hz, q, lfo_oct, rate_hz, stereo, shape, env_oct, sens_db, attack_ms, release_ms):
    """(g0, k, gmin, gmax, cl, ce, f, S, aA, 1 - aA, aR): the filter vertex' constants at rate sr, exactly the doubles the engine uses
    (host only).  kind: "lowpass" | "highpass" | "bandpass" | "notch"; shape: the chorus' names."""
    out = (C.c_double * 11)()
    _check(lib().td_filter_params(int(sr), filter_kind(kind), freq_hz, q, lfo_oct, rate_hz, stereo, chorus_shape(shape), env_oct, sens_db,
                                  attack_ms, release_ms, out, 11))
    return tuple(out[0:11])


def vocoder_params(sr, bands, lo_hz, hi_hz, q, response_ms, out_db):
    """(rows, a, g): the vocoder vertex' constants at rate sr, exactly the doubles the engine uses (host only) -- rows[b] = (f_b, b0,
    b1, b2, a1, a2) per band, a the follower's coefficient, g the output gain."""
    n = 6 * 16 + 2
    out = (C.c_double * n)()
    _check(lib().td_vocoder_params(int(sr), int(bands), lo_hz, hi_hz, q, response_ms, out_db, out, n))
    B = int(bands)
    return [tuple(out[6 * b:6 * b + 6]) for b in range(B)], out[6 * B], out[6 * B + 1]


def gate_params(sr, threshold_db, hysteresis_db, hold_ms, attack_ms, release_ms, range_db):
    """(To, Tc, H, aA, aR, F): the gate vertex' constants at rate sr, exactly the doubles the engine uses (host only; H an int)."""
    out = (C.c_double * 6)()
    _check(lib().td_gate_params(int(sr), threshold_db, hysteresis_db, hold_ms, attack_ms, release_ms, range_db, out))
    return (out[0], out[1], int(out[2]), out[3], out[4], out[5])


def _f3(v):
    """Three floats for a per-band parameter (low, mid, high)."""
    v = tuple(v)
    if len(v) != 3:
        raise ValueError("a multiband vertex takes three values per band parameter")
    return (C.c_float * 3)(*v)


def multiband_params(sr, lo_hz, hi_hz, threshold_db, ratio, attack_ms, release_ms, knee_db, makeup_db):
    """(sets, aA, aR): the multiband vertex' constants at rate sr, exactly the doubles the engine uses (host only) -- sets[s] = (b0, b1,
    b2, a1, a2) for s = L1, H1, L2, H2, A2."""
    out = (C.c_double * 27)()
    _check(lib().td_multiband_params(int(sr), lo_hz, hi_hz, _f3(threshold_db), _f3(ratio), attack_ms, release_ms, knee_db, _f3(makeup_db), out, 27))
    return [tuple(out[5 * s:5 * s + 5]) for s in range(5)], out[25], out[26]


def limiter_params(sr, ceiling_db, lookahead_ms, release_ms, drive_db):
    """(c, gin, L, a, latency): the limiter vertex' constants at rate sr, exactly the doubles the engine uses (host only; L and the
    latency, L - 1 frames, as ints)."""
    out = (C.c_double * 5)()
    _check(lib().td_limiter_params(int(sr), ceiling_db, lookahead_ms, release_ms, drive_db, out))
    return (out[0], out[1], int(out[2]), out[3], int(out[4]))


def convolution_params(sr, sample_len, length_ms, predelay_ms, out_db, norm):
    """(Lh, D, g, P, H, B): the convolution vertex' constants at rate sr for a response sample of sample_len frames, exactly as the
    engine uses them (host only) -- the response's frames, the pre-delay in frames, the trim before `norm`, the partitions, the
    frames the vertex carries (D + Lh - 1) and the partition length; all but g as ints."""
    out = (C.c_double * 6)()
    _check(lib().td_convolution_params(int(sr), int(sample_len), length_ms, predelay_ms, out_db, int(norm), out))
    return (int(out[0]), int(out[1]), out[2], int(out[3]), int(out[4]), int(out[5]))


def convolution_twiddles():
    """The twiddle table of the engine's transforms (host only): exp(-2 pi i j / 2048), j = 0 .. 1023, as complex128 -- the doubles the
    kernels read."""
    n = int(lib().td_convolution_twiddles(None, 0))
    out = (C.c_double * n)()
    lib().td_convolution_twiddles(out, n)
    a = np.frombuffer(out, dtype=np.float64).copy()
    return a[0::2] + 1j * a[1::2]


def chorus_params(sr, voices, delay_ms, depth_ms, rate_hz, stereo, shape):
    """The chorus vertex' constants at rate sr (host only), exactly as the engine uses them: (D0, A, f, H, s, Hch) -- the centre
    delay and the depth in frames, the LFO's cycles per frame, the frames of the line, the largest delay slope, and the gain the
    guard carries its estimate through the wet path at."""
    out = (C.c_double * 6)()
    _check(lib().td_chorus_params(int(sr), int(voices), delay_ms, depth_ms, rate_hz, stereo, chorus_shape(shape), out))
    return float(out[0]), float(out[1]), float(out[2]), int(out[3]), float(out[4]), float(out[5])


def reverb_params(sr, room, damp, width, size):
    """The reverb vertex' constants at rate sr (host only), exactly as the engine uses them: a dict with g, d1, d2, w1, w2, Hrev
    (the gain the guard carries its estimate through the wet path at), B (the window length at the default cap) and the line
    lengths in frames: combs_l, combs_r (8 each), allpass_l, allpass_r (4 each)."""
    out = (C.c_double * 31)()
    _check(lib().td_reverb_params(int(sr), room, damp, width, size, out))
    o = [float(x) for x in out]
    return {"g": o[0], "d1": o[1], "d2": o[2], "w1": o[3], "w2": o[4], "Hrev": o[5], "B": int(o[6]),
            "combs_l": [int(x) for x in o[7:15]], "combs_r": [int(x) for x in o[15:23]],
            "allpass_l": [int(x) for x in o[23:27]], "allpass_r": [int(x) for x in o[27:31]]}


def loudness_filters(sr):
    """The meter's filters at rate sr (host only): (shelf (b, a), high-pass (b, a)) as float64 arrays with a[0] = 1, and the
    true-peak FIR as a (phases, taps) float32 array (phase 0 the unit impulse)."""
    kw = (C.c_double * 10)()
    ph, taps = _sz(0), _sz(0)
    _check(lib().td_loudness_filters(int(sr), kw, None, 0, C.byref(ph), C.byref(taps)))
    fir = np.zeros((ph.value, taps.value), np.float32)
    _check(lib().td_loudness_filters(int(sr), kw, fir.ctypes.data_as(_fp), fir.size, C.byref(ph), C.byref(taps)))
    k = np.array(kw[:], np.float64)
    shelf = (k[0:3].copy(), np.array([1.0, k[3], k[4]]))
    hp = (k[5:8].copy(), np.array([1.0, k[8], k[9]]))
    return shelf, hp, fir


# -- mastering (include/termdaw_amd.h td_graph_master): TD_MASTER_FIELDS doubles per signal --
MASTER_FIELDS = LOUDNESS_FIELDS + ("input_integrated", "input_true_peak", "gain", "ceiling", "min_gain", "passes", "met")


def _master_dicts(out, n):
    rows = []
    for i in range(n):
        v = [float(x) for x in out[15 * i:15 * i + 15]]
        d = dict(zip(MASTER_FIELDS, v))
        d["frames"], d["sr"], d["passes"], d["met"] = int(v[6]), int(v[7]), int(v[13]), bool(v[14])
        rows.append(d)
    return rows


def master_f32(frames, sr, target_lufs, ceiling_dbtp=-1.0, lookahead_ms=5.0, release_ms=100.0):
    """Master host frames ((N, 2) float32, L R, at rate sr) on the device -> (mastered (N, 2) float32 frames, a dict of
    MASTER_FIELDS): the meter's figures of the result, the input's integrated loudness and true peak, the last pass' linear
    gain and internal ceiling, the smallest limiter gain, the passes run and whether both targets were met."""
    a = np.ascontiguousarray(frames, dtype=np.float32).reshape(-1, 2)
    res = np.zeros_like(a)
    out = (C.c_double * 15)()
    _check(lib().td_master_f32(a.ctypes.data_as(_fp), a.shape[0], int(sr), float(target_lufs), float(ceiling_dbtp),
                               float(lookahead_ms), float(release_ms), res.ctypes.data_as(_fp), out))
    return res, _master_dicts(out, 1)[0]


def device_count():
    return lib().td_device_count()


def set_device(i):
    _check(lib().td_set_device(i))


class SampleBank:
    def __init__(self, sample_rate, _handle=None):
        self.h = _handle or lib().td_samplebank_new(sample_rate)
        self._own = _handle is None
        self.sample_rate = sample_rate

    def __del__(self):
        if getattr(self, "h", None) and self._own:
            lib().td_samplebank_free(self.h)
            self.h = None

    def add_decoded(self, name, values, channels, sr, bits, method=""):
        a, p = _fa(values)
        _check(lib().td_samplebank_add_decoded(self.h, name.encode(), p, a.size, channels, sr, bits, method.encode()))

    def add(self, name, file, method=""):
        _check(lib().td_samplebank_add_file(self.h, name.encode(), file.encode(), method.encode()))

    def get_index(self, name):
        i = lib().td_samplebank_get_index(self.h, name.encode())
        return None if i < 0 else i

    def get_sample(self, index):
        n = lib().td_samplebank_sample_len(self.h, index)
        l = np.empty(n, np.float32)
        r = np.empty(n, np.float32)
        _check(lib().td_samplebank_read(self.h, index, l.ctypes.data_as(_fp), r.ctypes.data_as(_fp)))
        return l, r

    def get_max_sr_bd(self):
        a, b = _sz(), _sz()
        lib().td_samplebank_get_max_sr_bd(self.h, C.byref(a), C.byref(b))
        return a.value, b.value


class FlowwBank:
    def __init__(self, sr, bl, _handle=None):
        self.h = _handle or lib().td_flowwbank_new(sr, bl)
        self._own = _handle is None

    def __del__(self):
        if getattr(self, "h", None) and self._own:
            lib().td_flowwbank_free(self.h)
            self.h = None

    def add_events(self, name, events):
        ev = np.ascontiguousarray(np.asarray(events, dtype=np.float32).reshape(-1, 3))
        return lib().td_flowwbank_add_events(self.h, name.encode(), ev.ctypes.data_as(C.POINTER(td_event)), ev.shape[0])

    def add_midi(self, name, path):
        """FlowwBank::add_floww (floww.rs:40-48); raises TermdawError like the reference's Err."""
        i = lib().td_flowwbank_add_midi(self.h, name.encode(), str(path).encode())
        if i < 0:
            raise TermdawError(last_error())
        return i

    def declare_stream(self, name):
        return lib().td_flowwbank_declare_stream(self.h, name.encode())

    def append_stream(self, name, events):
        ev = np.ascontiguousarray(np.asarray(events, dtype=np.float32).reshape(-1, 3))
        return lib().td_flowwbank_append_stream(self.h, name.encode(), ev.ctypes.data_as(C.POINTER(td_event)), ev.shape[0])

    def trim_streams(self):
        lib().td_flowwbank_trim_streams(self.h)

    def get_events(self, index):
        n = lib().td_flowwbank_get_events(self.h, index, None, 0)
        buf = np.zeros((max(n, 1), 3), np.float32)
        lib().td_flowwbank_get_events(self.h, index, buf.ctypes.data_as(C.POINTER(td_event)), n)
        return buf[:n]

    def get_index(self, name):
        i = lib().td_flowwbank_get_index(self.h, name.encode())
        return None if i < 0 else i

    def set_time(self, t):
        lib().td_flowwbank_set_time(self.h, t)

    def set_time_to_next_block(self):
        lib().td_flowwbank_set_time_to_next_block(self.h)


class Graph:
    def __init__(self, bl, sr, _handle=None):
        self.h = _handle or lib().td_graph_new(bl, sr)
        self._own = _handle is None
        self.bl = bl
        self.sr = sr

    def __del__(self):
        if getattr(self, "h", None) and self._own:
            lib().td_graph_free(self.h)
            self.h = None

    def add_sum(self, name, gain, angle):
        _check(lib().td_graph_add_sum(self.h, name.encode(), gain, angle))

    def add_normalize(self, name, gain, angle):
        _check(lib().td_graph_add_normalize(self.h, name.encode(), gain, angle))

    def add_sampleloop(self, name, gain, angle, sample_index):
        _check(lib().td_graph_add_sampleloop(self.h, name.encode(), gain, angle, sample_index))

    def add_sample_multi(self, name, gain, angle, sample_index, floww_index, note):
        _check(lib().td_graph_add_sample_multi(self.h, name.encode(), gain, angle, sample_index, floww_index, note))

    def add_sample_lerp(self, name, gain, angle, sample_index, floww_index, note, lerp_len):
        _check(lib().td_graph_add_sample_lerp(self.h, name.encode(), gain, angle, sample_index, floww_index, note, lerp_len))

    def add_debug_sine(self, name, gain, angle, floww_index):
        _check(lib().td_graph_add_debug_sine(self.h, name.encode(), gain, angle, floww_index))

    def add_synth(self, name, gain, angle, floww_index, sq_vel, sq_z, sq_adsr, tf_vel, tf_z, tf_adsr, tr_vel, tr_adsr):
        a1, p1 = _fa(sq_adsr)
        a2, p2 = _fa(tf_adsr)
        a3, p3 = _fa(tr_adsr)
        _check(lib().td_graph_add_synth(self.h, name.encode(), gain, angle, floww_index, sq_vel, sq_z, p1, a1.size,
                                        tf_vel, tf_z, p2, a2.size, tr_vel, p3, a3.size))

    def add_sampsyn(self, name, gain, angle, floww_index, adsr, table_bytes):
        a, p = _fa(adsr)
        tb = bytes(table_bytes) if table_bytes is not None else None
        _check(lib().td_graph_add_sampsyn(self.h, name.encode(), gain, angle, floww_index, p, a.size, tb, len(tb) if tb else 0))

    def add_adsr(self, name, gain, angle, wet, floww_index, use_off, use_max, note, adsr):
        a, p = _fa(adsr)
        _check(lib().td_graph_add_adsr(self.h, name.encode(), gain, angle, wet, floww_index, int(use_off), int(use_max),
                                       note, p, a.size))

    def add_bandpass(self, name, gain, angle, wet, lo_hz, hi_hz, pass_):
        _check(lib().td_graph_add_bandpass(self.h, name.encode(), gain, angle, wet, lo_hz, hi_hz, int(pass_)))

    def add_compressor(self, name, gain, angle, wet, threshold_db, ratio, attack_ms, release_ms, knee_db, makeup_db):
        """A feed-forward compressor vertex (this engine's own; the definition is in include/termdaw_amd.h)."""
        _check(lib().td_graph_add_compressor(self.h, name.encode(), gain, angle, wet, threshold_db, ratio, attack_ms, release_ms,
                                             knee_db, makeup_db))

    def add_eq(self, name, gain, angle, wet, kind, freq_hz, q, gain_db):
        """A parametric EQ vertex (this engine's own; the definition is in include/termdaw_amd.h).  kind: a name of EQ_KINDS or
        its TD_EQ_* index."""
        _check(lib().td_graph_add_eq(self.h, name.encode(), gain, angle, wet, eq_kind(kind), freq_hz, q, gain_db))

    def add_delay(self, name, gain, angle, wet, time_ms, feedback, cross):
        """A feedback delay (echo) vertex (this engine's own; the definition is in include/termdaw_amd.h)."""
        _check(lib().td_graph_add_delay(self.h, name.encode(), gain, angle, wet, time_ms, feedback, cross))

    def add_saturator(self, name, gain, angle, wet, kind, drive_db, bias, out_db, oversample):
        """An oversampled waveshaper vertex (this engine's own; the definition is in include/termdaw_amd.h).  kind: a name of
        SAT_KINDS or its TD_SAT_* index; oversample: 1, 2, 4 or 8.  The vertex has a latency of 64 frames when oversample > 1."""
        _check(lib().td_graph_add_saturator(self.h, name.encode(), gain, angle, wet, sat_kind(kind), drive_db, bias, out_db, int(oversample)))

    def add_chorus(self, name, gain, angle, wet, voices, delay_ms, depth_ms, rate_hz, stereo, shape):
        """A chorus vertex: LFO-modulated fractional delay lines (this engine's own; the definition is in include/termdaw_amd.h).
        voices: 1 .. 4; shape: a name of CHORUS_SHAPES or its TD_CHORUS_* index.  The vertex has no latency."""
        _check(lib().td_graph_add_chorus(self.h, name.encode(), gain, angle, wet, int(voices), delay_ms, depth_ms, rate_hz, stereo, chorus_shape(shape)))

    def add_reverb(self, name, gain, angle, wet, room, damp, width, size):
        """A reverb vertex: 8 damped feedback combs and 4 all-pass sections per channel (this engine's own; the definition is in
        include/termdaw_amd.h).  room, damp, width: [0, 1]; size: [0.5, 2], a factor on every line's length."""
        _check(lib().td_graph_add_reverb(self.h, name.encode(), gain, angle, wet, room, damp, width, size))

    def add_gate(self, name, gain, angle, wet, threshold_db, hysteresis_db, hold_ms, attack_ms, release_ms, range_db):
        """A noise gate vertex: hysteresis, hold and an attack / release fade (this engine's own; the definition is in
        include/termdaw_amd.h)."""
        _check(lib().td_graph_add_gate(self.h, name.encode(), gain, angle, wet, threshold_db, hysteresis_db, hold_ms, attack_ms, release_ms,
                                       range_db))

    def add_phaser(self, name, gain, angle, wet, stages, lo_hz, hi_hz, rate_hz, feedback, stereo, shape):
        """A phaser vertex: a swept all-pass chain with feedback (this engine's own; the definition is in include/termdaw_amd.h).
        stages 2 | 4 | 6 | 8; shape "sine" or "triangle" (or the chorus' constants)."""
        _check(lib().td_graph_add_phaser(self.h, name.encode(), gain, angle, wet, int(stages), lo_hz, hi_hz, rate_hz, feedback, stereo,
                                         chorus_shape(shape)))

    def add_vocoder(self, name, gain, angle, wet, bands, lo_hz, hi_hz, q, response_ms, out_db):
        """A vocoder vertex: a keyed band-pass bank (this engine's own; the definition is in include/termdaw_amd.h).  bands 4 | 8 |
        16; its inputs are the carrier, its key edges (connect_key) the modulator."""
        _check(lib().td_graph_add_vocoder(self.h, name.encode(), gain, angle, wet, int(bands), lo_hz, hi_hz, q, response_ms, out_db))

    def add_filter(self, name, gain, angle, wet, kind, freq_hz, q, lfo_oct, rate_hz, stereo, shape, env_oct, sens_db, attack_ms, release_ms):
        """A filter vertex: a state-variable filter swept by an LFO and an envelope follower (this engine's own; the definition is in
        include/termdaw_amd.h).  kind "lowpass" | "highpass" | "bandpass" | "notch"; shape "sine" or "triangle" (or the constants);
        its key edges (connect_key) feed the follower."""
        _check(lib().td_graph_add_filter(self.h, name.encode(), gain, angle, wet, filter_kind(kind), freq_hz, q, lfo_oct, rate_hz, stereo,
                                         chorus_shape(shape), env_oct, sens_db, attack_ms, release_ms))

    def add_limiter(self, name, gain, angle, wet, ceiling_db, lookahead_ms, release_ms, drive_db):
        """A limiter vertex: a lookahead brickwall limiter, L - 1 frames of latency (this engine's own; the definition is in
        include/termdaw_amd.h)."""
        _check(lib().td_graph_add_limiter(self.h, name.encode(), gain, angle, wet, ceiling_db, lookahead_ms, release_ms, drive_db))

    def add_multiband(self, name, gain, angle, wet, lo_hz, hi_hz, threshold_db, ratio, attack_ms, release_ms, knee_db, makeup_db):
        """A multiband vertex: a three-way Linkwitz-Riley crossover into three band compressors (this engine's own; the definition is
        in include/termdaw_amd.h).  threshold_db, ratio and makeup_db: three values each, for the low, mid and high band."""
        _check(lib().td_graph_add_multiband(self.h, name.encode(), gain, angle, wet, lo_hz, hi_hz, _f3(threshold_db), _f3(ratio), attack_ms,
                                            release_ms, knee_db, _f3(makeup_db)))

    def add_convolution(self, name, gain, angle, wet, sample_index, length_ms, predelay_ms, out_db, norm):
        """A convolution vertex: the bank's sample at sample_index as an impulse response, by partitioned FFT (this engine's own; the
        definition is in include/termdaw_amd.h)."""
        _check(lib().td_graph_add_convolution(self.h, name.encode(), gain, angle, wet, int(sample_index), length_ms, predelay_ms, out_db, int(norm)))

    def connect(self, a, b):
        return bool(lib().td_graph_connect(self.h, a.encode(), b.encode()))

    def connect_key(self, a, b):
        """A key edge (sidechain) from any vertex a to a compressor, gate, vocoder or filter vertex b: b takes its level (a vocoder: its
        modulator) from the sum of its key sources and goes on processing the sum of its inputs (include/termdaw_amd.h td_graph_connect_key).  False: last_error()."""
        return bool(lib().td_graph_connect_key(self.h, a.encode(), b.encode()))

    def set_output(self, name):
        return bool(lib().td_graph_set_output(self.h, name.encode()))

    def check_graph(self):
        return bool(lib().td_graph_check(self.h))

    def set_time(self, t):
        lib().td_graph_set_time(self.h, t)

    def change_time(self, delta, plus):
        return lib().td_graph_change_time(self.h, delta, int(plus))

    def get_time(self):
        return lib().td_graph_get_time(self.h)

    def reset_normalize_vertices(self):
        lib().td_graph_reset_normalize_vertices(self.h)

    def get_normalization_value(self, name):
        return lib().td_graph_get_normalization_value(self.h, name.encode())

    def render(self, sb, fb):
        """Graph::render: one block at the playhead -> (l, r) or None."""
        l = np.empty(self.bl, np.float32)
        r = np.empty(self.bl, np.float32)
        ok = lib().td_graph_render_block(self.h, sb.h, fb.h, l.ctypes.data_as(_fp), r.ctypes.data_as(_fp))
        if ok < 0:
            raise TermdawError(last_error())
        if not ok:
            return None
        return l, r

    def true_normalize_scan(self, sb, fb, chunks):
        _check(lib().td_graph_normalize_scan(self.h, sb.h, fb.h, chunks))

    def render_all(self, sb, fb, cs, bd=16, want_f32=True, want_pcm=True):
        """State::render loop on the GPU. Returns (pcm[frames,2], f32[frames,2])."""
        n = lib().td_graph_render_all(self.h, sb.h, fb.h, cs, bd)
        if cs and not n:
            raise TermdawError(last_error())
        frames = cs * self.bl
        self._pcm_shape = (frames, np.int32 if bd > 16 else np.int16)
        pcm = f = None
        if want_pcm:
            pcm = np.zeros((frames, 2), np.int32 if bd > 16 else np.int16)
            if frames:
                _check(lib().td_graph_read_pcm(self.h, pcm.ctypes.data_as(_vp), pcm.nbytes))
        if want_f32:
            f = np.zeros((frames, 2), np.float32)
            if frames:
                _check(lib().td_graph_read_f32(self.h, f.ctypes.data_as(_fp), f.size))
        return pcm, f

    def render_all_resampled(self, sb, fb, cs, bd, psr, render_sr):
        """State::render, psr > render_sr arm (build-defined resampler). Returns (pcm, f32)."""
        n = lib().td_graph_render_all_resampled(self.h, sb.h, fb.h, cs, bd, psr, render_sr)
        if cs and not n:
            raise TermdawError(last_error())
        self._pcm_shape = (n, np.int32 if bd > 16 else np.int16)
        pcm = np.zeros((n, 2), np.int32 if bd > 16 else np.int16)
        f = np.zeros((n, 2), np.float32)
        if n:
            _check(lib().td_graph_read_pcm(self.h, pcm.ctypes.data_as(_vp), pcm.nbytes))
            _check(lib().td_graph_read_f32(self.h, f.ctypes.data_as(_fp), f.size))
        return pcm, f

    # -- bench hooks --
    def render_all_async(self, sb, fb, cs, bd=16):
        n = lib().td_graph_render_all_async(self.h, sb.h, fb.h, cs, bd)
        if cs and not n:
            raise TermdawError(last_error())
        self._pcm_shape = (n, np.int32 if bd > 16 else np.int16)
        return n

    # -- stems: named vertices rendered to PCM of their own by the same render (include/termdaw_amd.h) --
    def set_stems(self, names):
        """Replaces the stem list (an empty list clears it); an unknown or repeated name raises and leaves the list as it was."""
        arr, n = _names(names)
        _check(lib().td_graph_set_stems(self.h, arr, n))

    def stem_count(self):
        return lib().td_graph_stem_count(self.h)

    def read_stem_pcm(self, i):
        """Stem i of this Graph object's last render_all / render_all_resampled / render_all_async: (frames, 2) of the output's dtype."""
        frames, dt = getattr(self, "_pcm_shape", (None, None))
        if frames is None:
            raise TermdawError("read_stem_pcm: nothing rendered through this Graph object")
        pcm = np.zeros((frames, 2), dt)
        if frames:
            _check(lib().td_graph_read_stem_pcm(self.h, i, pcm.ctypes.data_as(_vp), pcm.nbytes))
        return pcm

    def stem_peak(self, i):
        """max |x| of the frames of stem i quantised in the last render (NaN when a frame was NaN)."""
        v = lib().td_graph_stem_peak(self.h, i)
        if v == 0.0 and not lib().td_graph_stem_pcm_device(self.h, i):   # (0.0 is also what the call returns for a stem not rendered)
            raise TermdawError(last_error())
        return float(v)

    def sync(self):
        _check(lib().td_graph_sync(self.h))

    def norm_fix_runs(self):
        """How often a single-pass Normalize launch was redone by the check kernel after the fact (0 in normal operation)."""
        return lib().td_graph_norm_fix_runs(self.h)

    def norm_respec(self):
        """Blocks the single-pass Normalize launches stored a second time since the last call (counted only with engine option
        debug.norm bit 2 or bit 4 set; include/termdaw_amd.h)."""
        return lib().td_graph_norm_respec(self.h)

    def host_times(self, reset=True):
        """Host ms per phase since the last reset: compile, descriptors, upload, launches; and chunk count."""
        out = (C.c_double * 4)()
        n = lib().td_graph_host_times(self.h, out, int(reset))
        return {"compile": out[0], "descriptors": out[1], "upload": out[2], "launch": out[3], "chunks": n}

    def set_profiling(self, on):
        lib().td_graph_set_profiling(self.h, int(on))

    def kernel_times(self):
        cap = 64   # (a level with every effect kind in it takes more than 32 launch families)
        names = (_cp * cap)()
        ms = (C.c_float * cap)()
        cnt = (_sz * cap)()
        n = lib().td_graph_last_kernel_times(self.h, names, ms, cnt, cap)
        return {names[i].decode(): (ms[i], cnt[i]) for i in range(n)}

    def output_peak(self):
        return lib().td_graph_output_peak(self.h)

    def device_bytes(self):
        return lib().td_graph_device_bytes(self.h)

    def band_stats(self):
        out = (C.c_uint32 * 3)()
        _check(lib().td_graph_band_stats(self.h, out))
        return {"mismatched": out[0], "recomputed": out[1], "parked": out[2]}

    def loudness(self, stems=True):
        """Loudness of the last whole render (render_all / render_all_async / render_all_resampled): the output, then with
        stems=True every stem it wrote, in ONE launch -> a list of dicts of LOUDNESS_FIELDS."""
        n = 1 + (int(lib().td_graph_stem_count(self.h)) if stems else 0)
        if stems and n > 1 and not lib().td_graph_stem_pcm_device(self.h, n - 2):
            n = 1   # (stems set since the render: it wrote none)
        out = (C.c_double * (8 * n))()
        _check(lib().td_graph_loudness(self.h, out, n))
        self._loud_n = n
        return _loudness_dicts(out, n)

    def read_pcm(self, frames=None, bd=None):
        """The output's words of the last whole render as they are now (after master(): mastered), frames x 2; frames and bd
        default to those of this object's last render_all / render_all_resampled."""
        if frames is None or bd is None:
            f, dt = self._pcm_shape
            frames = f if frames is None else frames
            bd = (32 if dt == np.int32 else 16) if bd is None else bd
        out = np.zeros((frames, 2), np.int32 if bd > 16 else np.int16)
        if frames:
            _check(lib().td_graph_read_pcm(self.h, out.ctypes.data_as(_vp), out.nbytes))
        return out

    def master(self, target_lufs, ceiling_dbtp=-1.0, lookahead_ms=5.0, release_ms=100.0):
        """Master the last whole render in place to target_lufs under ceiling_dbtp (from the rendered words every time: calls
        never compound) -> a dict of MASTER_FIELDS.  read_pcm / loudness() see the mastered words; stems and f32 frames do not."""
        out = (C.c_double * 15)()
        _check(lib().td_graph_master(self.h, float(target_lufs), float(ceiling_dbtp), float(lookahead_ms), float(release_ms), out))
        return _master_dicts(out, 1)[0]

    def momentary(self, which=0):
        """The 400 ms block series (LUFS) of signal `which` (0 the output, 1 + i stem i) of the last loudness() call."""
        if not 0 <= which < getattr(self, "_loud_n", 0):
            raise TermdawError("momentary: signal %d was not measured by this Graph object's last loudness()" % which)
        n = lib().td_graph_momentary(self.h, which, None, 0)
        out = np.zeros(n, np.float64)
        if n:
            lib().td_graph_momentary(self.h, which, out.ctypes.data_as(C.POINTER(C.c_double)), n)
        return out

    def band_guard_stats(self):
        """band_mode 2: renders audited, renders done again with the exact kernels, last / largest estimated RMS deviation."""
        out = (C.c_double * 4)()
        _check(lib().td_graph_band_guard_stats(self.h, out))
        return {"audits": int(out[0]), "redos": int(out[1]), "last_est": out[2], "max_est": out[3]}

    def set_option(self, key, value):
        _check(lib().td_graph_set_option(self.h, key.encode(), int(value)))

    def get_option(self, key):
        v = _lng(0)
        _check(lib().td_graph_get_option(self.h, key.encode(), C.byref(v)))
        return int(v.value)


COMM_ID_BYTES = 128
_HOST_ALLREDUCE = C.CFUNCTYPE(_i32, _vp, _fp, _sz)


def comm_unique_id():
    """rank 0: the 128-byte id every rank hands to Comm (ncclGetUniqueId behind td_comm_unique_id)."""
    buf = (C.c_char * COMM_ID_BYTES)()
    _check(lib().td_comm_unique_id(buf, COMM_ID_BYTES))
    return bytes(buf)


class Comm:
    """The ranks of a multi-GPU job (td_comm): `Comm(unique_id, rank, world)` joins over RCCL on the current device;
    `Comm.over_host(fn, rank, world)` runs the same exchange over the host's own all-reduce -- fn(table: np.float32[n]) replaces
    the table in place by its element-wise maximum over the ranks (MPI hosts; two ranks on one GPU in tests)."""

    def __init__(self, unique_id=None, rank=0, world=1, _h=None, _keep=None):
        self._keep = _keep
        if _h is not None:
            self.h = _h
        else:
            if unique_id is None or len(unique_id) < COMM_ID_BYTES:
                raise ValueError("Comm needs the 128-byte id of comm_unique_id()")
            self.h = lib().td_comm_init(bytes(unique_id), len(unique_id), rank, world)
        if not self.h:
            raise TermdawError(last_error())
        self.rank, self.world = rank, world

    @classmethod
    def over_host(cls, fn, rank, world):
        def tramp(_ctx, table, n):
            try:
                fn(np.ctypeslib.as_array(table, shape=(n,)))
                return 1
            except Exception:   # (an exception must not cross the C ABI: the entry reports a failed exchange)
                return 0
        cb = _HOST_ALLREDUCE(tramp)
        h = lib().td_comm_init_host(C.cast(cb, _vp), None, rank, world)
        return cls(rank=rank, world=world, _h=h, _keep=cb)

    def backend(self):
        return lib().td_comm_backend(self.h).decode()

    def __del__(self):
        if getattr(self, "h", None):
            lib().td_comm_free(self.h)
            self.h = None


def comm_library():
    return lib().td_comm_library().decode()


class Batch:
    """Many independent projects rendered together on one GPU (BASELINE config 5): State::render's loop
    (state.rs:563-575) for every project, same-kind launches of different projects merged into one grid."""

    def __init__(self):
        self.h = lib().td_batch_new()
        self.projects = []   # (sb, fb, g) kept alive: the batch only borrows the handles

    def __del__(self):
        if getattr(self, "h", None):
            lib().td_batch_free(self.h)
            self.h = None

    def add(self, sb, fb, g):
        i = lib().td_batch_add(self.h, g.h, sb.h, fb.h)
        if i < 0:
            raise TermdawError(last_error())
        self.projects.append((sb, fb, g))
        return i

    def __len__(self):
        return lib().td_batch_size(self.h)

    def rewind(self):
        lib().td_batch_rewind(self.h)

    def render_all(self, cs, bd=16):
        n = lib().td_batch_render_all(self.h, cs, bd)
        if cs and len(self) and not n:
            raise TermdawError(last_error())
        return n

    def render_all_async(self, cs, bd=16):
        n = lib().td_batch_render_all_async(self.h, cs, bd)
        if cs and len(self) and not n:
            raise TermdawError(last_error())
        return n

    def sync(self):
        _check(lib().td_batch_sync(self.h))

    E2E_KEYS = ("wall_ms", "setup_ms", "gpu_render_span_ms", "copy_span_ms", "copy_busy_ms", "bytes", "write_span_ms", "enqueue_ms")

    def render_to_files(self, cs, bd=16, render_sr=48000, paths=None, group=4, writers=8):
        """State::render end to end for every project: render -> page-locked host PCM -> WAV files, pipelined.  paths None:
        no files (render + D2H).  Returns the timing report (E2E_KEYS)."""
        arr = None
        if paths is not None:
            arr = (_cp * len(paths))(*[p.encode() for p in paths])
        times = (C.c_double * 8)()
        _check(lib().td_batch_render_to_files(self.h, cs, bd, render_sr, arr, group, writers if paths is not None else 0, times))
        return dict(zip(self.E2E_KEYS, [float(x) for x in times]))

    def host_pcm(self, i, bd=16):
        """Project i's PCM of the last render_to_files, copied out of the library's page-locked buffer."""
        n = _sz(0)
        p = lib().td_batch_host_pcm(self.h, i, C.byref(n))
        if not p:
            raise TermdawError("no host PCM")
        raw = C.string_at(p, n.value)
        return np.frombuffer(raw, dtype=np.int32 if bd > 16 else np.int16).reshape(-1, 2).copy()

    def normalize_scan(self, chunks):
        _check(lib().td_batch_normalize_scan(self.h, chunks))

    def loudness(self):
        """Loudness of every project's last render in ONE launch (Graph.loudness's dict per project, td_batch_add order)."""
        out = (C.c_double * (8 * max(len(self), 1)))()
        _check(lib().td_batch_loudness(self.h, out))
        return _loudness_dicts(out, len(self))

    def master(self, target_lufs, ceiling_dbtp=-1.0, lookahead_ms=5.0, release_ms=100.0):
        """Graph.master on every project's last render, each pass of all projects in one launch per kernel -> a list of dicts."""
        out = (C.c_double * (15 * max(len(self), 1)))()
        _check(lib().td_batch_master(self.h, float(target_lufs), float(ceiling_dbtp), float(lookahead_ms), float(release_ms), out))
        return _master_dicts(out, len(self))

    def peaks(self):
        out = np.zeros(max(len(self), 1), np.float32)
        _check(lib().td_batch_peaks(self.h, out.ctypes.data_as(_fp)))
        return out[:len(self)]

    def exchange_peaks(self, comm, per_rank):
        """The job's one collective (td_batch_exchange_peaks): this rank's peaks into the per_rank x world table, then ONE
        all-reduce(max) on the batch's stream -- enqueued, not waited for (sync() does).  comm None: a job of one rank."""
        _check(lib().td_batch_exchange_peaks(self.h, comm.h if comm is not None else None, per_rank))

    def peak_table(self, n=None):
        """The exchanged table, copied to the host (synchronises)."""
        cnt = _sz(0)
        lib().td_batch_peak_table(self.h, C.byref(cnt))
        n = cnt.value if n is None else n
        out = np.zeros(max(n, 1), np.float32)
        _check(lib().td_batch_read_peak_table(self.h, out.ctypes.data_as(_fp), n))
        return out[:n]

    def peak_table_device(self, device_ptr, n_total, first=0, stride=1):
        """Fills n_total floats at `device_ptr` (e.g. torch_tensor.data_ptr()): own entries at first + i*stride, 0 elsewhere."""
        _check(lib().td_batch_peak_table_device(self.h, C.c_void_p(device_ptr), n_total, first, stride))

    def read_pcm(self, i, cs, bd=16):
        sb, fb, g = self.projects[i]
        pcm = np.zeros((cs * g.bl, 2), np.int32 if bd > 16 else np.int16)
        if pcm.size:
            _check(lib().td_graph_read_pcm(g.h, pcm.ctypes.data_as(_vp), pcm.nbytes))
        return pcm

    def set_profiling(self, on):
        lib().td_batch_set_profiling(self.h, int(on))

    def kernel_times(self):
        cap = 64   # (a level with every effect kind in it takes more than 32 launch families)
        names = (_cp * cap)()
        ms = (C.c_float * cap)()
        cnt = (_sz * cap)()
        n = lib().td_batch_last_kernel_times(self.h, names, ms, cnt, cap)
        return {names[i].decode(): (ms[i], cnt[i]) for i in range(n)}

    def mark(self, which):
        """A mark on the batch's stream: 0 before a run of submissions, 1 behind it (marked_ms: device time between them)."""
        _check(lib().td_batch_mark(self.h, int(which)))

    def marked_ms(self):
        return float(lib().td_batch_marked_ms(self.h))

    def host_times(self, reset=True):
        out = (C.c_double * 4)()
        n = lib().td_batch_host_times(self.h, out, int(reset))
        return {"compile": out[0], "descriptors": out[1], "upload": out[2], "launch": out[3], "steps": n}


class State:
    """State (state.rs:27-578): project script -> banks + graph -> render to WAV."""

    def __init__(self, wdir="", project_samplerate=44100, buffer_length=1024, open_dir=None):
        if open_dir is not None:
            self.h = lib().td_state_open(open_dir.encode())
        else:
            self.h = lib().td_state_new(wdir.encode(), project_samplerate, buffer_length)
        if not self.h:
            raise TermdawError(last_error())

    def __del__(self):
        if getattr(self, "h", None):
            lib().td_state_free(self.h)
            self.h = None

    def refresh(self, source=None):
        ok = lib().td_state_refresh(self.h) if source is None else lib().td_state_refresh_source(self.h, source.encode())
        return bool(ok)

    def set_option(self, key, value):
        """Engine option of the State's graph; a State defaults to band_mode 2 (the scan under the guard), set_option("band_mode", 0) = exact."""
        _check(lib().td_state_set_option(self.h, key.encode(), int(value)))

    def scan_exact(self):
        _check(lib().td_state_scan_exact(self.h))

    def render(self, path=None):
        """State::render; with stems set, each stem X also goes to "<path minus .wav>.<X>.wav"."""
        _check(lib().td_state_render(self.h, path.encode() if path else None))

    def set_stems(self, names):
        """Stems of the following renders, resolved at each render (an unknown name fails it before any file is written)."""
        arr, n = _names(names)
        _check(lib().td_state_set_stems(self.h, arr, n))

    def set_master(self, target_lufs=None, ceiling_dbtp=-1.0):
        """Master every following render to target_lufs under ceiling_dbtp (default lookahead and release); None: off."""
        on = target_lufs is not None
        _check(lib().td_state_set_master(self.h, int(on), float(target_lufs) if on else 0.0, float(ceiling_dbtp)))

    def master_report(self):
        """The MASTER_FIELDS dict of the last render, or None when it was not mastered."""
        out = (C.c_double * 15)()
        return _master_dicts(out, 1)[0] if lib().td_state_master_report(self.h, out) else None

    def render_to_memory(self):
        nbytes = lib().td_state_render_to_memory(self.h, None, 0)
        bd = self.bd
        out = np.zeros(nbytes // (4 if bd > 16 else 2), np.int32 if bd > 16 else np.int16)
        if nbytes:
            if not lib().td_state_render_to_memory(self.h, out.ctypes.data_as(_vp), out.nbytes):
                raise TermdawError(last_error())
        return out.reshape(-1, 2)

    def render_view(self):
        """Render and return the PCM as a read-only numpy view of the library's page-locked read-back buffer
        (frames x 2; valid until the next render of this State)."""
        n = _sz(0)
        p = lib().td_state_render_view(self.h, C.byref(n))
        if not p:
            raise TermdawError(last_error())
        dt = np.int32 if self.bd > 16 else np.int16
        if n.value == 0:
            return np.zeros((0, 2), dt)
        buf = (C.c_uint8 * n.value).from_address(p)
        out = np.frombuffer(buf, dtype=dt).reshape(-1, 2)
        out.flags.writeable = False
        return out

    @property
    def cs(self):
        return lib().td_state_chunk_count(self.h)

    @property
    def render_sr(self):
        return lib().td_state_render_samplerate(self.h)

    @property
    def bd(self):
        return lib().td_state_bitdepth(self.h)

    @property
    def output_file(self):
        return lib().td_state_output_file(self.h).decode()

    def dump_calls(self):
        return lib().td_state_dump_calls(self.h).decode()

    @property
    def g(self):
        return Graph(lib().td_state_buffer_length(self.h), lib().td_state_project_samplerate(self.h),
                     _handle=lib().td_state_graph(self.h))

    @property
    def sb(self):
        return SampleBank(lib().td_state_project_samplerate(self.h), _handle=lib().td_state_samplebank(self.h))

    @property
    def fb(self):
        return FlowwBank(lib().td_state_project_samplerate(self.h), lib().td_state_buffer_length(self.h),
                         _handle=lib().td_state_flowwbank(self.h))
