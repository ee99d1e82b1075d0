"""
ctypes binding of libshaderflow_hip.so (include/shaderflow_hip.h) — the only way the host package reaches
the GPU. There is NO CPU fallback: if the library is missing, or no device is visible when a context is
created, the product path raises.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import numpy as np

PACKAGE = Path(__file__).resolve().parent
LIBRARY = PACKAGE/"libshaderflow_hip.so"

OK = 0
U8, F32, U16, F16 = 0, 1, 2, 3
NEAREST, LINEAR = 0, 1
T_FLOAT, T_INT, T_BOOL, T_VEC2, T_VEC3, T_VEC4, T_MAT2, T_MAT3, T_MAT4 = range(9)
TAPE_SPECTROGRAM, TAPE_WAVEFORM, TAPE_UNIFORMS, TAPE_TARGETS, TAPE_LOUDNESS, TAPE_SCROLL, TAPE_STATE = range(7)
E_UNSUPPORTED = -4
E_TOO_LARGE = -6

Handle = C.c_uint64


def source_fingerprint() -> str:
    """sha256 over the kernel sources the library is built from (csrc/): ties profiles under profiles/ to the code they measured"""
    import hashlib
    digest = hashlib.sha256()
    for path in sorted((PACKAGE/"csrc").iterdir()):
        if path.suffix in (".hip", ".hpp", ".inc") or path.name == "Makefile":
            digest.update(path.name.encode())
            digest.update(path.read_bytes())
    return digest.hexdigest()[:16]


class CtxInfo(C.Structure):
    _fields_ = [("device_name", C.c_char*128), ("gcn_arch", C.c_char*64), ("device_id", C.c_int32),
                ("compute_units", C.c_int32), ("max_texture_dim", C.c_int32), ("wavefront_size", C.c_int32),
                ("total_memory", C.c_int64), ("lds_per_cu", C.c_int64)]


class DynCoeffF32(C.Structure):
    _fields_ = [("dt", C.c_float), ("k1", C.c_float), ("k2", C.c_float), ("k3", C.c_float)]


class DynCoeffF64(C.Structure):
    _fields_ = [("dt", C.c_double), ("k1", C.c_double), ("k2", C.c_double), ("k3", C.c_double)]


class FrameClock(C.Structure):
    _fields_ = [("iTime", C.c_float), ("iTau", C.c_float), ("iSpectrogramOffset", C.c_float), ("iFrame", C.c_int32)]


class SequencePass(C.Structure):
    _fields_ = [("program", Handle), ("kind", C.c_int), ("matrix", C.c_int), ("target", Handle), ("ssaa", C.c_int), ("subsample", C.c_int)]


class SequenceMatrix(C.Structure):
    _fields_ = [("temporal", C.c_int), ("layers", C.c_int), ("textures", C.POINTER(Handle)), ("names", C.POINTER(C.c_char_p))]


class ClockTick(C.Structure):
    _fields_ = [("time", C.c_float), ("tau", C.c_float), ("deltatime", C.c_float), ("frame", C.c_int32)]


PASS_LAYERS, PASS_FUSED, PASS_RESOLVE = 0, 1, 2
VIDEO_RGB24, VIDEO_I420, VIDEO_MJPEG, VIDEO_PNG, VIDEO_PLANAR = 0, 1, 2, 3, 4


class PlanarLayout(C.Structure):
    """sfx_planar_layout (include/shaderflow_hip.h): the SFX_PLANAR_* numbers of a planar source's layout (planarsource.PlanarLayout.native)"""
    _fields_ = [("subsampling", C.c_int32), ("depth", C.c_int32), ("matrix", C.c_int32), ("range", C.c_int32), ("filter", C.c_int32),
                ("siting", C.c_int32)]


class PianoParams(C.Structure):
    _fields_ = [("time_offset", C.c_double), ("roll_time", C.c_double), ("lookahead", C.c_double), ("release_before_end", C.c_double)]


class PianoTick(C.Structure):
    _fields_ = [("time", C.c_double), ("coeff", DynCoeffF32), ("dynamic", C.c_float*2), ("previous_is_target", C.c_int32), ("reserved", C.c_int32)]


class Sequence(C.Structure):
    """sfx_sequence (include/shaderflow_hip.h), field for field: the tables, the sink, the optional tape, the optional piano, the optional video, and whether
    the video may stand beside the other two (`video_join`, zero unless a caller sets it)"""
    _fields_ = [("passes", C.POINTER(SequencePass)), ("npasses", C.c_int), ("matrices", C.POINTER(SequenceMatrix)), ("nmatrices", C.c_int),
                ("clock", C.POINTER(ClockTick)), ("nframes", C.c_int),
                ("ring", Handle), ("first_slot", C.c_int), ("fd", C.c_int), ("planar_slots", C.POINTER(C.c_void_p)),
                ("yuv_matrix", C.c_int), ("width", C.c_int), ("height", C.c_int),
                ("tape", Handle), ("tape_frame0", C.c_int),
                ("piano", Handle), ("piano_ticks", C.POINTER(PianoTick)), ("piano_dynamic_name", C.c_char_p),
                ("video", Handle), ("video_slots", C.POINTER(C.c_int32)), ("video_names", C.POINTER(C.c_char_p)),
                ("video_join", C.c_int32)]


class Binding(C.Structure):
    """sfx_binding (include/shaderflow_hip.h): a uniform or sampler name of a loaded program"""
    _fields_ = [("name", C.c_char_p), ("sampler", C.c_int), ("slot", C.c_int), ("count", C.c_int), ("integer", C.c_int)]


class TapeDesc(C.Structure):
    _fields_ = [("points", C.c_int32), ("chunk_size", C.c_int32), ("reducer", C.c_int32), ("volume_window", C.c_int32),
                ("use_mfma", C.c_int32), ("volume_integrate", C.c_int32), ("std_integrate", C.c_int32),
                ("length_samples", C.c_int32), ("precision", C.c_double)]


# name → (restype, argtypes); every symbol declared in include/shaderflow_hip.h
P = C.POINTER
PROTOTYPES: dict[str, tuple] = {
    "sfx_last_error": (C.c_char_p, []),
    "sfx_version": (C.c_char_p, []),
    "sfx_abi_layout": (C.c_uint64, []),
    "sfx_last_kernel": (C.c_char_p, []),
    "sfx_ctx_create": (C.c_int, [C.c_int, C.c_void_p, P(Handle)]),
    "sfx_ctx_info": (C.c_int, [Handle, P(CtxInfo)]),
    "sfx_ctx_synchronize": (C.c_int, [Handle]),
    "sfx_ctx_output_top_down": (C.c_int, [Handle, C.c_int]),
    "sfx_ctx_filter_model": (C.c_int, [Handle, C.c_int]),
    "sfx_ctx_copy_streams": (C.c_int, [Handle, P(C.c_int), P(C.c_int)]),
    "sfx_ctx_tile_misses": (C.c_int, [Handle, P(C.c_ulonglong)]),
    "sfx_ctx_destroy": (C.c_int, [Handle]),
    "sfx_event_record": (C.c_int, [Handle, C.c_int]),
    "sfx_event_elapsed_ms": (C.c_int, [Handle, C.c_int, C.c_int, P(C.c_float)]),
    "sfx_texture_create": (C.c_int, [Handle, C.c_int, C.c_int, C.c_int, C.c_int, P(Handle)]),
    "sfx_texture_params": (C.c_int, [Handle, C.c_int, C.c_int, C.c_int]),
    "sfx_texture_write": (C.c_int, [Handle, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int]),
    "sfx_texture_read": (C.c_int, [Handle, C.c_void_p, C.c_size_t]),
    "sfx_texture_build_mipmaps": (C.c_int, [Handle]),
    "sfx_texture_read_level": (C.c_int, [Handle, C.c_int, C.c_void_p, C.c_size_t]),
    "sfx_texture_device_ptr": (C.c_int, [Handle, P(C.c_void_p), P(C.c_size_t)]),
    "sfx_texture_destroy": (C.c_int, [Handle]),
    "sfx_program_lookup": (C.c_int, [Handle, C.c_char_p, P(Handle), P(C.c_int)]),
    "sfx_program_load": (C.c_int, [Handle, C.c_void_p, C.c_size_t, P(Binding), C.c_int, P(Handle)]),
    "sfx_program_name": (C.c_char_p, [Handle]),
    "sfx_program_fusable": (C.c_int, [Handle, C.c_int]),
    "sfx_uniform_set": (C.c_int, [Handle, C.c_char_p, C.c_int, C.c_void_p, P(C.c_int)]),
    "sfx_sampler_bind": (C.c_int, [Handle, C.c_char_p, Handle, P(C.c_int)]),
    "sfx_sampler_bind_many": (C.c_int, [Handle, P(C.c_char_p), P(Handle), C.c_int]),
    "sfx_uniform_set_clock": (C.c_int, [Handle, C.c_float, C.c_float, C.c_float, C.c_int]),
    "sfx_program_destroy": (C.c_int, [Handle]),
    "sfx_render": (C.c_int, [Handle, Handle, C.c_int]),
    "sfx_resolve": (C.c_int, [Handle, Handle, Handle, C.c_int]),
    "sfx_render_resolve": (C.c_int, [Handle, Handle, C.c_int, C.c_int]),
    "sfx_fused_supported": (C.c_int, [C.c_int, C.c_int]),
    "sfx_ring_create": (C.c_int, [Handle, C.c_size_t, C.c_int, P(Handle)]),
    "sfx_ring_read_async": (C.c_int, [Handle, Handle, C.c_int]),
    "sfx_ring_read_device_async": (C.c_int, [Handle, C.c_void_p, C.c_int]),
    "sfx_ring_fence": (C.c_int, [Handle, C.c_int]),
    "sfx_ring_read_fenced_async": (C.c_int, [Handle, C.c_void_p, C.c_int, C.c_int]),
    "sfx_ring_pipe_frames": (C.c_int, [Handle, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int]),
    "sfx_ring_stream_wait": (C.c_int, [Handle, C.c_int]),
    "sfx_ring_sync": (C.c_int, [Handle, C.c_int, P(C.c_void_p)]),
    "sfx_ring_pipe": (C.c_int, [Handle, C.c_int, C.c_int]),
    "sfx_ring_pipe_sync": (C.c_int, [Handle, C.c_int]),
    "sfx_ring_destroy": (C.c_int, [Handle]),
    "sfx_ring_create_sized": (C.c_int, [Handle, C.c_size_t, C.c_int, C.c_int, P(Handle)]),
    "sfx_ring_sizes": (C.c_int, [Handle, P(C.c_uint32), C.c_size_t, P(C.c_size_t)]),
    "sfx_ring_side_track": (C.c_int, [Handle, C.c_void_p, C.c_size_t, P(C.c_uint64), C.c_size_t]),
    "sfx_ring_segments": (C.c_int, [Handle, C.c_uint64, C.c_uint64, C.c_uint32]),
    "sfx_ring_segment_cuts": (C.c_int, [Handle, P(C.c_uint32), C.c_size_t, P(C.c_size_t)]),
    "sfx_jpeg_create": (C.c_int, [Handle, C.c_int, C.c_int, C.c_int, P(Handle)]),
    "sfx_jpeg_destroy": (C.c_int, [Handle]),
    "sfx_jpeg_encode": (C.c_int, [Handle, C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "sfx_jpeg_header": (C.c_int, [Handle, C.c_void_p, P(C.c_size_t)]),
    "sfx_jpeg_coefficients": (C.c_int, [Handle, P(C.c_int16)]),
    "sfx_png_create": (C.c_int, [Handle, C.c_int, C.c_int, P(Handle)]),
    "sfx_png_destroy": (C.c_int, [Handle]),
    "sfx_png_encode": (C.c_int, [Handle, C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "sfx_png_capacity": (C.c_int, [C.c_int, C.c_int, P(C.c_size_t)]),
    "sfx_png_filtered": (C.c_int, [Handle, P(C.c_uint8)]),
    "sfx_png_code_lengths": (C.c_int, [Handle, P(C.c_uint32), P(C.c_uint8), P(C.c_int)]),
    "sfx_rgb_to_yuv420": (C.c_int, [Handle, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]),
    "sfx_peer_export": (C.c_int, [Handle, C.c_void_p, C.c_void_p]),
    "sfx_peer_open": (C.c_int, [Handle, C.c_void_p, P(C.c_void_p)]),
    "sfx_peer_close": (C.c_int, [Handle, C.c_void_p]),
    "sfx_peer_copy": (C.c_int, [Handle, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]),
    "sfx_peer_fence": (C.c_int, [Handle, C.c_int]),
    "sfx_peer_flush": (C.c_int, [Handle]),
    "sfx_peer_route": (C.c_int, [Handle, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]),
    "sfx_shm_create": (C.c_int, [Handle, C.c_char_p, C.c_int, C.c_int, C.c_size_t, C.c_int, P(Handle)]),
    "sfx_shm_push": (C.c_int, [Handle, C.c_void_p]),
    "sfx_shm_flush": (C.c_int, [Handle]),
    "sfx_shm_wait": (C.c_int, [Handle, C.c_int64]),
    "sfx_shm_drain": (C.c_int, [Handle, C.c_int, P(C.c_int32), P(C.c_int32), C.c_int]),
    "sfx_shm_drain_wait": (C.c_int, [Handle]),
    "sfx_shm_abort": (C.c_int, [Handle]),
    "sfx_shm_unlink": (C.c_int, [Handle]),
    "sfx_shm_destroy": (C.c_int, [Handle]),
    "sfx_flac_info": (C.c_int, [C.c_void_p, C.c_size_t, P(C.c_int64), P(C.c_int), P(C.c_int), P(C.c_int)]),
    "sfx_flac_decode": (C.c_int, [C.c_void_p, C.c_size_t, P(C.c_float), C.c_int64, P(C.c_int64)]),
    "sfx_audio_upload": (C.c_int, [Handle, P(C.c_float), C.c_int64, C.c_int, C.c_int, P(Handle)]),
    "sfx_audio_destroy": (C.c_int, [Handle]),
    "sfx_stft_plan": (C.c_int, [Handle, C.c_int, C.c_int, C.c_int, C.c_int, P(C.c_int32), P(C.c_int32), P(C.c_float), P(Handle)]),
    "sfx_stft_plan_resampled": (C.c_int, [Handle, C.c_int, C.c_int, P(C.c_int32), P(C.c_int32), P(C.c_double), C.c_int, C.c_int, C.c_int,
                                          P(C.c_int32), P(C.c_int32), P(C.c_float), P(Handle)]),
    "sfx_stft_plan_magnitude": (C.c_int, [Handle, C.c_int]),
    "sfx_stft_plan_window": (C.c_int, [Handle, P(C.c_double), C.c_int]),
    "sfx_stft_plan_destroy": (C.c_int, [Handle]),
    "sfx_stft_power": (C.c_int, [Handle, Handle, P(C.c_int64), C.c_int, P(C.c_float)]),
    "sfx_stft_spectrum": (C.c_int, [Handle, Handle, P(C.c_int64), C.c_int, P(C.c_double)]),
    "sfx_filterbank_apply": (C.c_int, [Handle, P(C.c_float), C.c_int, C.c_int, P(C.c_float)]),
    "sfx_spectrogram_targets": (C.c_int, [Handle, Handle, P(C.c_int64), C.c_int, C.c_int, P(C.c_float)]),
    "sfx_waveform_rows": (C.c_int, [Handle, P(C.c_int64), C.c_int, C.c_int, C.c_int, C.c_int, P(C.c_float)]),
    "sfx_volume_std": (C.c_int, [Handle, P(C.c_int64), C.c_int, C.c_int, P(C.c_float)]),
    "sfx_dynamics_scan": (C.c_int, [Handle, C.c_int, C.c_int, P(C.c_float), P(DynCoeffF32), C.c_float, P(C.c_float), P(C.c_float)]),
    "sfx_dynamics_scan_f64": (C.c_int, [Handle, C.c_int, C.c_int, P(C.c_double), P(DynCoeffF64), C.c_double, C.c_int, P(C.c_double), P(C.c_double)]),
    "sfx_tape_create": (C.c_int, [Handle, Handle, P(TapeDesc), C.c_int, P(Handle)]),
    "sfx_clock_tape_create": (C.c_int, [Handle, C.c_int, P(Handle)]),
    "sfx_tape_reset": (C.c_int, [Handle]),
    "sfx_tape_snapshot": (C.c_int, [Handle, C.c_int]),
    "sfx_tape_build": (C.c_int, [Handle, C.c_int, P(C.c_int64), P(FrameClock), P(DynCoeffF32), P(DynCoeffF64), P(DynCoeffF64)]),
    "sfx_tape_read": (C.c_int, [Handle, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t]),
    "sfx_tape_destroy": (C.c_int, [Handle]),
    "sfx_render_tape": (C.c_int, [Handle, Handle, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "sfx_piano_create": (C.c_int, [Handle, P(C.c_int32), P(C.c_int32), P(C.c_double), P(C.c_double), P(C.c_float), P(C.c_float), C.c_int, P(PianoParams),
                                   Handle, Handle, Handle, P(C.c_float), P(Handle)]),
    "sfx_piano_step": (C.c_int, [Handle, C.c_double, P(DynCoeffF32), C.c_int]),
    "sfx_piano_state_read": (C.c_int, [Handle, P(C.c_float)]),
    "sfx_piano_destroy": (C.c_int, [Handle]),
    "sfx_video_create": (C.c_int, [Handle, P(Handle), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, P(Handle)]),
    "sfx_video_slot": (C.c_int, [Handle, C.c_int, P(C.c_void_p), P(C.c_size_t)]),
    "sfx_video_submit": (C.c_int, [Handle, C.c_int]),
    "sfx_video_step": (C.c_int, [Handle, C.c_int]),
    "sfx_video_destroy": (C.c_int, [Handle]),
    "sfx_video_create_mjpeg": (C.c_int, [Handle, P(Handle), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_int, P(Handle)]),
    "sfx_video_submit_bytes": (C.c_int, [Handle, C.c_int, C.c_size_t]),
    "sfx_video_status": (C.c_int, [Handle, C.c_int, P(C.c_int64), P(C.c_uint32)]),
    "sfx_jpeg_decode": (C.c_int, [Handle, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, P(C.c_uint32)]),
    "sfx_jpeg_decode_sync": (C.c_int, [Handle, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                       P(C.c_uint32), P(C.c_uint32)]),
    "sfx_video_jpeg_paths": (C.c_int, [Handle, P(C.c_uint64), P(C.c_uint64)]),
    "sfx_video_create_png": (C.c_int, [Handle, P(Handle), C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_int, P(Handle)]),
    "sfx_video_png_paths": (C.c_int, [Handle, P(C.c_uint64), P(C.c_uint64)]),
    "sfx_video_create_planar": (C.c_int, [Handle, P(Handle), C.c_int, C.c_int, C.c_int, P(PlanarLayout), C.c_int, P(Handle)]),
    "sfx_png_decode": (C.c_int, [Handle, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, P(C.c_uint32), P(C.c_uint32)]),
    "sfx_sequence_run": (C.c_int, [Handle, P(Sequence)]),
    "sfx_device_alloc": (C.c_int, [Handle, C.c_size_t, P(C.c_void_p)]),
    "sfx_device_free": (C.c_int, [Handle, C.c_void_p]),
    "sfx_device_copy": (C.c_int, [Handle, C.c_void_p, C.c_void_p, C.c_size_t]),
    "sfx_device_read": (C.c_int, [Handle, C.c_void_p, C.c_void_p, C.c_size_t]),
}

_lib: C.CDLL | None = None


class NativeError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"libshaderflow_hip: {message} (code {code})")
        self.code = code


def lib() -> C.CDLL:
    """Loads the HIP library; raises ImportError when it has not been built (no fallback exists)."""
    global _lib
    if _lib is None:
        path = Path(os.environ.get("SHADERFLOW_HIP_LIBRARY", LIBRARY))
        if not path.exists():
            raise ImportError(
                f"{path} is missing: build it with `make -C shaderflow_amd/csrc` "
                f"(or `python -c 'import __graft_entry__ as g; g.build()'`). There is no CPU fallback."
            )
        L = C.CDLL(str(path), mode=C.RTLD_GLOBAL)
        for name, (restype, argtypes) in PROTOTYPES.items():
            fn = getattr(L, name)             # AttributeError if the header and the library disagree
            fn.restype = restype
            fn.argtypes = argtypes
        _lib = L
    return _lib


def check(code: int) -> None:
    if code != OK:
        raise NativeError(code, lib().sfx_last_error().decode("utf-8", "replace"))


def as_ptr(array: np.ndarray, ctype):
    return array.ctypes.data_as(C.POINTER(ctype))


NUMPY_DTYPES = {np.dtype(np.uint8): U8, np.dtype(np.float32): F32, np.dtype(np.uint16): U16, np.dtype(np.float16): F16}


class Context:
    """One HIP device + one stream (the GL context of scene.py:145-157)"""

    def __init__(self, device: int = 0, stream: int | None = None):
        self.handle = Handle()
        check(lib().sfx_ctx_create(device, C.c_void_p(stream) if stream else None, C.byref(self.handle)))
        self.device = device

    def info(self) -> CtxInfo:
        info = CtxInfo()
        check(lib().sfx_ctx_info(self.handle, C.byref(info)))
        return info

    def synchronize(self) -> None:
        check(lib().sfx_ctx_synchronize(self.handle))

    def copy_streams(self) -> tuple[int, int]:
        """(streams looked at, of which in series with the render stream) when the context's two copy streams were chosen"""
        candidates, colliding = C.c_int(), C.c_int()
        check(lib().sfx_ctx_copy_streams(self.handle, C.byref(candidates), C.byref(colliding)))
        return candidates.value, colliding.value

    def tile_misses(self) -> int:
        """Blocks of the LDS-tiled visualizer kernels that ran the generic taps since the previous call (the first call starts the count)"""
        blocks = C.c_ulonglong()
        check(lib().sfx_ctx_tile_misses(self.handle, C.byref(blocks)))
        return blocks.value

    def filter_model(self, model: str | int) -> None:
        """How LINEAR unorm8 textures of this context are filtered (sfx_ctx_filter_model): "spec" — float weights, the default — or
        "llvmpipe" / "fixed8": the 8-bit fixed-point filter of the software rasteriser the reference's CPU path runs on"""
        code = {"spec": 0, "float": 0, "llvmpipe": 1, "fixed8": 1}.get(model.strip().lower()) if isinstance(model, str) else int(model)
        if code is None:
            raise ValueError(f"filter model {model!r}: 'spec' or 'llvmpipe'")
        check(lib().sfx_ctx_filter_model(self.handle, code))

    def output_top_down(self, enabled: bool) -> None:
        check(lib().sfx_ctx_output_top_down(self.handle, 1 if enabled else 0))

    def event_record(self, slot: int) -> None:
        check(lib().sfx_event_record(self.handle, slot))

    def event_elapsed_ms(self, start: int, stop: int) -> float:
        ms = C.c_float()
        check(lib().sfx_event_elapsed_ms(self.handle, start, stop, C.byref(ms)))
        return ms.value

    def alloc(self, nbytes: int) -> int:
        ptr = C.c_void_p()
        check(lib().sfx_device_alloc(self.handle, nbytes, C.byref(ptr)))
        return ptr.value

    def free(self, ptr: int) -> None:
        check(lib().sfx_device_free(self.handle, C.c_void_p(ptr)))

    def rgb_to_yuv420(self, rgb: int, yuv: int, width: int, height: int, frames: int = 1, matrix: int = 0) -> None:
        """`frames` consecutive RGB8 frames on the device → planar yuv420p on the device (sfx_rgb_to_yuv420), on the context's stream"""
        check(lib().sfx_rgb_to_yuv420(self.handle, C.c_void_p(rgb), C.c_void_p(yuv), width, height, frames, matrix))

    def copy(self, dst: int, src: int, nbytes: int) -> None:
        check(lib().sfx_device_copy(self.handle, C.c_void_p(dst), C.c_void_p(src), nbytes))

    # peer windows (sharded export, "device-sdma")
    def peer_export(self, ptr: int) -> bytes:
        handle = C.create_string_buffer(64)
        check(lib().sfx_peer_export(self.handle, C.c_void_p(ptr), handle))
        return handle.raw

    def peer_route(self) -> dict:
        """How this context's peer copies travel: {"route": "sdma-engines" | "hip-streams" | None, "engines": [ids], "copies", "bytes"}"""
        via, ids, copies, nbytes = C.c_int(), (C.c_int*2)(), C.c_ulonglong(), C.c_ulonglong()
        check(lib().sfx_peer_route(self.handle, C.byref(via), ids, C.byref(copies), C.byref(nbytes)))
        route = {1: "sdma-engines", 0: "hip-streams"}.get(via.value)
        return {"route": route, "engines": [int(i) for i in ids] if via.value == 1 else [], "copies": int(copies.value), "bytes": int(nbytes.value)}

    def peer_open(self, handle: bytes) -> int:
        ptr = C.c_void_p()
        check(lib().sfx_peer_open(self.handle, C.create_string_buffer(handle, 64), C.byref(ptr)))
        return ptr.value

    def peer_close(self, ptr: int) -> None:
        check(lib().sfx_peer_close(self.handle, C.c_void_p(ptr)))

    def peer_copy(self, remote: int, local: int, nbytes: int, lane: int = 0) -> None:
        check(lib().sfx_peer_copy(self.handle, C.c_void_p(remote), C.c_void_p(local), nbytes, lane))

    def peer_fence(self, lane: int) -> None:
        check(lib().sfx_peer_fence(self.handle, lane))

    def peer_flush(self) -> None:
        check(lib().sfx_peer_flush(self.handle))

    def read(self, ptr: int, nbytes: int) -> np.ndarray:
        out = np.empty(nbytes, np.uint8)
        check(lib().sfx_device_read(self.handle, C.c_void_p(ptr), out.ctypes.data, nbytes))
        return out

    def destroy(self) -> None:
        if self.handle.value:
            lib().sfx_ctx_destroy(self.handle)
            self.handle = Handle()


class JpegEncoder:
    """Motion-JPEG encoder of one context and one picture size (sfx_jpeg_*): RGB8 frames on the device → sink frames on the device"""
    SINK_HEADER = 64

    def __init__(self, context: Context, width: int, height: int, quality: int = 90):
        self.context, self.width, self.height, self.quality = context, width, height, quality
        self.handle = Handle()
        check(lib().sfx_jpeg_create(context.handle, width, height, quality, C.byref(self.handle)))
        self.mcus_x, self.mcus_y = (width + 15)//16, (height + 15)//16
        self.sink_bytes = self.SINK_HEADER + self.mcus_x*self.mcus_y*768

    def encode(self, rgb: int, sink: int, frames: int = 1, bottom_up: bool = False) -> None:
        check(lib().sfx_jpeg_encode(self.handle, C.c_void_p(rgb), C.c_void_p(sink), frames, 1 if bottom_up else 0))

    def header(self) -> bytes:
        count = C.c_size_t(2048)
        buffer = C.create_string_buffer(count.value)
        check(lib().sfx_jpeg_header(self.handle, buffer, C.byref(count)))
        return buffer.raw[:count.value]

    def coefficients(self) -> np.ndarray:
        out = np.empty((self.mcus_y, self.mcus_x, 6, 64), np.int16)
        check(lib().sfx_jpeg_coefficients(self.handle, as_ptr(out, C.c_int16)))
        return out

    def destroy(self) -> None:
        if self.handle.value:
            lib().sfx_jpeg_destroy(self.handle)
            self.handle = Handle()


class PngEncoder:
    """PNG encoder of one context and one picture size (sfx_png_*): RGB8 frames on the device → sink frames on the device, each a complete PNG file"""
    SINK_HEADER = 64

    def __init__(self, context: Context, width: int, height: int):
        self.context, self.width, self.height = context, width, height
        self.sink_bytes = self.SINK_HEADER + self.capacity(width, height)
        self.handle = Handle()
        check(lib().sfx_png_create(context.handle, width, height, C.byref(self.handle)))

    @staticmethod
    def capacity(width: int, height: int) -> int:
        """Payload bytes of a sink frame: no picture of this size encodes to more (sfx_png_capacity)"""
        count = C.c_size_t()
        check(lib().sfx_png_capacity(width, height, C.byref(count)))
        return count.value

    def encode(self, rgb: int, sink: int, frames: int = 1, bottom_up: bool = False) -> None:
        check(lib().sfx_png_encode(self.handle, C.c_void_p(rgb), C.c_void_p(sink), frames, 1 if bottom_up else 0))

    def filtered(self) -> np.ndarray:
        out = np.empty((self.height, 1 + 3*self.width), np.uint8)
        check(lib().sfx_png_filtered(self.handle, as_ptr(out, C.c_uint8)))
        return out

    @staticmethod
    def code_lengths(context: Context, histogram) -> tuple[np.ndarray, bool]:
        """The code-length step on a 316-entry histogram → (the dynamic code's 316 lengths, whether the block takes the fixed codes)"""
        counts = np.ascontiguousarray(histogram, np.uint32)
        if counts.shape != (316,):
            raise ValueError(f"a histogram has 286 + 30 counts, not {counts.shape}")
        lengths, fixed = np.empty(316, np.uint8), C.c_int()
        check(lib().sfx_png_code_lengths(context.handle, as_ptr(counts, C.c_uint32), as_ptr(lengths, C.c_uint8), C.byref(fixed)))
        return lengths, bool(fixed.value)

    def destroy(self) -> None:
        if self.handle.value:
            lib().sfx_png_destroy(self.handle)
            self.handle = Handle()


_default_context: Context | None = None


def default_context() -> Context:
    """Process-wide context on LOCAL_RANK's device (one process per GPU)"""
    global _default_context
    if _default_context is None:
        _default_context = Context(int(os.environ.get("LOCAL_RANK", "0")))
    return _default_context
