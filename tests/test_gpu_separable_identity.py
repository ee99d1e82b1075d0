"""
The separable unit (launch_separable.hip: bars.frag, waveform.frag and default.glsl on per-frame column and row tables) pinned byte for
byte: which kernel a launch gets (sfx_last_kernel) and the CRC-32 of the frame it writes.

TABLE was recorded on the commit BEFORE k_separable_fused's three bodies were separated from their shared row walk and the unit's
picker became a list of instances; the unit must reproduce it byte for byte. It is data, never regenerated from the code under test:
a deliberate change of a pixel edits the rows it moves, by hand, with the reason.

Shapes are the smallest that reach each path. Every fragment gets a frame narrower than a block of 256 pixels, one exactly a block
wide, a full and a partial block with w % 4 == 0 (the packed 12-byte stores beside the per-byte tail) and with an odd w, heights below
a group of four rows and heights that end a walk of 8 rows with a single row (9, 17, 33), both row orders, both final.glsl kernels.
bars / waveform: widths that are multiples of four run as k_separable_runs and, with SHADERFLOW_SEPARABLE_RUNS=0, as
k_separable_fused; the spectrogram carries the non-finite and extreme entries of
test_gpu_pixels.py::test_separable_audio_fragments_equal_the_generic_fused_kernel. default.glsl: the identity camera, a zoomed and
panned one, iCameraZoom = 0.2 (columns out of bounds), iTau 0.0 (the singular line on the diagonal), 0.31, 0.77, and the two passes
of SHADERFLOW_DEFAULT_QUADS=1. The tall frames reach the instances no small launch takes (2 048 blocks and more): default.glsl's
16-row walk at 516 x 10933 (2 052 blocks; the last walk is one group and one row) against its 8-row walk at 516 x 10912 (2 046) — the
two evaluate the polar terms at different points, so their bytes differ —, and the 32-row walks of bars / waveform at 21 829 rows with
per-byte tails (517 wide) and packed stores (516 wide). Where an instance's bytes do not depend on its row count (bars, waveform) the
static_asserts beside the picker pin the choice, not this test.

No multi-frame launch is pinned here: the one helper the suite has for it (tape_run of test_gpu_tape_parity.py) does not fit at a small
size. Four frames of 260 x 37 per launch came out with the same device audio tape every time, yet the LAST frame's bytes changed with what
the process had run before — also for k_separable_runs<bars>, whose device code is instruction for instruction the recorded commit's —
so such a row says nothing about this unit. blockIdx.z and the per-frame tables stay covered by test_gpu_tape_parity.py (bars and
waveform, 60 frames per launch, against the oracle).
"""
import zlib

import numpy as np
import pytest

from shaderflow_amd import _native as N
from tests.helpers import Gpu, gpu_bind_all, visualizer_inputs

pytestmark = pytest.mark.gpu

SWITCHES = ("SHADERFLOW_SEPARABLE", "SHADERFLOW_SEPARABLE_RUNS", "SHADERFLOW_DEFAULT_QUADS")
FUSED, RUNS_OFF, QUADS = {}, {"SHADERFLOW_SEPARABLE_RUNS": "0"}, {"SHADERFLOW_DEFAULT_QUADS": "1"}

CAMERAS = {
    "identity": dict(),
    "zoomed": dict(iCameraZoom=1.4, iCameraPosition=(0.2, -0.1, 0.0)),
    "wide": dict(iCameraZoom=0.2),                                  # columns out of bounds
}

# (fragment, w, h, subsample, top_down, (camera, iTau) for default.glsl or the spectrogram's gain, switches, sfx_last_kernel, CRC-32 of the frame)
TABLE = [
    ('default', 4, 1, 2, False, ('identity', 0.0), FUSED, 'k_separable_fused<default>', 0xe442ff62),
    ('default', 255, 3, 1, True, ('zoomed', 0.31), FUSED, 'k_separable_fused<default>', 0x683a0ee6),
    ('default', 256, 8, 2, False, ('wide', 0.77), FUSED, 'k_separable_fused<default>', 0xe29289fd),
    ('default', 257, 9, 2, True, ('identity', 0.0), FUSED, 'k_separable_fused<default>', 0x66de06a6),
    ('default', 260, 17, 1, False, ('zoomed', 0.0), FUSED, 'k_separable_fused<default>', 0x8c87740c),
    ('default', 516, 33, 2, True, ('identity', 0.31), FUSED, 'k_separable_fused<default>', 0x4237fc01),
    ('default', 260, 37, 2, False, ('wide', 0.0), FUSED, 'k_separable_fused<default>', 0x68d87d23),
    ('default', 516, 7, 1, True, ('zoomed', 0.77), FUSED, 'k_separable_fused<default>', 0xb139bf32),
    ('default', 516, 37, 2, False, ('identity', 0.77), FUSED, 'k_separable_fused<default>', 0x8e907285),
    ('default', 257, 33, 1, True, ('wide', 0.31), FUSED, 'k_separable_fused<default>', 0xe9ed3787),
    ('default', 256, 37, 2, False, ('identity', 0.31), QUADS, 'k_separable_fused<default>', 0x7c2a08a1),
    ('default', 516, 21, 2, True, ('zoomed', 0.0), QUADS, 'k_separable_fused<default>', 0x2727a7f2),
    ('default', 260, 4, 1, False, ('identity', 0.77), QUADS, 'k_separable_fused<default>', 0x8e10906b),
    ('bars', 4, 1, 2, False, 3.0, FUSED, 'k_separable_runs<bars>', 0xcca39ea7),
    ('bars', 4, 1, 2, False, 3.0, RUNS_OFF, 'k_separable_fused<bars>', 0xcca39ea7),
    ('bars', 255, 3, 1, True, 40.0, FUSED, 'k_separable_fused<bars>', 0x8a0519dc),
    ('bars', 256, 8, 2, False, 0.2, FUSED, 'k_separable_runs<bars>', 0xb3971a28),
    ('bars', 256, 8, 2, False, 0.2, RUNS_OFF, 'k_separable_fused<bars>', 0xe2f33ef1),
    ('bars', 257, 9, 2, True, 3.0, FUSED, 'k_separable_fused<bars>', 0xbc93e8d7),
    ('bars', 260, 17, 1, False, 0.5, FUSED, 'k_separable_runs<bars>', 0x01866c35),
    ('bars', 260, 17, 1, False, 0.5, RUNS_OFF, 'k_separable_fused<bars>', 0x28b8458e),
    ('bars', 516, 33, 2, True, 3.0, FUSED, 'k_separable_runs<bars>', 0x8b2a12a2),
    ('bars', 516, 33, 2, True, 3.0, RUNS_OFF, 'k_separable_fused<bars>', 0x58d28db8),
    ('bars', 260, 37, 2, False, 40.0, FUSED, 'k_separable_runs<bars>', 0x2bf78e94),
    ('bars', 260, 37, 2, False, 40.0, RUNS_OFF, 'k_separable_fused<bars>', 0x2bf78e94),
    ('bars', 516, 7, 1, True, 0.2, FUSED, 'k_separable_runs<bars>', 0x8e40ce5e),
    ('bars', 516, 7, 1, True, 0.2, RUNS_OFF, 'k_separable_fused<bars>', 0xce226ede),
    ('waveform', 4, 1, 2, False, 3.0, FUSED, 'k_separable_runs<waveform>', 0xec93baff),
    ('waveform', 4, 1, 2, False, 3.0, RUNS_OFF, 'k_separable_fused<waveform>', 0xec93baff),
    ('waveform', 255, 3, 1, True, 40.0, FUSED, 'k_separable_fused<waveform>', 0x986d4e0b),
    ('waveform', 256, 8, 2, False, 0.2, FUSED, 'k_separable_runs<waveform>', 0xe8bf1843),
    ('waveform', 256, 8, 2, False, 0.2, RUNS_OFF, 'k_separable_fused<waveform>', 0xe8bf1843),
    ('waveform', 257, 9, 2, True, 3.0, FUSED, 'k_separable_fused<waveform>', 0x00227c6a),
    ('waveform', 260, 17, 1, False, 0.5, FUSED, 'k_separable_runs<waveform>', 0x475798d6),
    ('waveform', 260, 17, 1, False, 0.5, RUNS_OFF, 'k_separable_fused<waveform>', 0x475798d6),
    ('waveform', 516, 33, 2, True, 3.0, FUSED, 'k_separable_runs<waveform>', 0x108e78a4),
    ('waveform', 516, 33, 2, True, 3.0, RUNS_OFF, 'k_separable_fused<waveform>', 0x108e78a4),
    ('waveform', 260, 37, 2, False, 40.0, FUSED, 'k_separable_runs<waveform>', 0x87885ae1),
    ('waveform', 260, 37, 2, False, 40.0, RUNS_OFF, 'k_separable_fused<waveform>', 0x87885ae1),
    ('waveform', 516, 7, 1, True, 0.2, FUSED, 'k_separable_runs<waveform>', 0x5cab9843),
    ('waveform', 516, 7, 1, True, 0.2, RUNS_OFF, 'k_separable_fused<waveform>', 0x5cab9843),
    ('default', 516, 10933, 2, False, ('identity', 0.31), FUSED, 'k_separable_fused<default>', 0xf440a49e),
    ('default', 516, 10912, 2, False, ('identity', 0.31), FUSED, 'k_separable_fused<default>', 0x2a7e088e),
    ('bars', 517, 21829, 2, True, 3.0, FUSED, 'k_separable_fused<bars>', 0xf4f5e9d6),
    ('bars', 516, 21829, 2, False, 3.0, RUNS_OFF, 'k_separable_fused<bars>', 0x8081692f),
    ('waveform', 517, 21829, 2, True, 3.0, FUSED, 'k_separable_fused<waveform>', 0xf20cf0d1),
    ('waveform', 516, 21829, 2, False, 3.0, RUNS_OFF, 'k_separable_fused<waveform>', 0xfb796ecf),
]

def _id(row):
    return "-".join(str(v) for v in row[:6]) + "".join(f"-{k[11:]}={v}" for k, v in row[6].items())


@pytest.fixture()
def gpu():
    g = Gpu()
    yield g
    g.close()


def render_row(gpu, monkeypatch, name, w, h, subsample, top_down, setting, switches):
    """One frame of the table: (sfx_last_kernel, CRC-32 of its bytes)"""
    u, arrays, params = visualizer_inputs(w, h, seed=77, volume=0.6)
    u.iSSAA = 2.0
    prog, _ = gpu.program(name)
    if name == "default":
        camera, u.iTau = setting
        for key, value in CAMERAS[camera].items():
            cur = getattr(u, key)
            if hasattr(cur, "__len__"):
                for i, v in enumerate(value):
                    cur[i] = v
            else:
                setattr(u, key, value)
        gpu.set_uniforms(prog, u)
        gpu_bind_all(gpu, prog, arrays, params)
    else:
        spectrogram = arrays["iSpectrogram"].astype(np.float32)*setting
        flat = spectrogram.reshape(-1)
        flat[3] = -1.0; flat[10] = np.inf; flat[17] = np.nan; flat[24] = 0.0; flat[31] = 120.0**2; flat[38] = np.float32(120.0**2)*np.float32(0.25)
        arrays["iSpectrogram"] = spectrogram
        gpu.set_uniforms(prog, u)
        for key in ("iSpectrogram", "iWaveform"):
            gpu.bind(prog, key + "0x0", gpu.texture(arrays[key], *params[key]))
    for key in SWITCHES:
        monkeypatch.delenv(key, raising=False)
    for key, value in switches.items():
        monkeypatch.setenv(key, value)
    N.check(gpu.lib.sfx_ctx_output_top_down(gpu.ctx.handle, int(top_down)))
    try:
        frame = gpu.render_resolve(prog, w, h, 2, subsample)
    finally:
        N.check(gpu.lib.sfx_ctx_output_top_down(gpu.ctx.handle, 0))
    return gpu.lib.sfx_last_kernel().decode(), zlib.crc32(frame.tobytes())


@pytest.mark.parametrize("row", TABLE, ids=_id)
def test_separable_frame_is_the_recorded_one(gpu, monkeypatch, row):
    assert render_row(gpu, monkeypatch, *row[:7]) == row[7:]
