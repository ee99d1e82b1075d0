"""
The cases of tests/test_gpu_layered.py (k_multipass_layer1 / k_motionblur_layer1 against the oracle) and the oracle-side halves of
them, shared with tests/test_host_layered.py, which checks without a GPU that the cases still bite.

Layer contents are white noise (any misplaced texel shows), row 0 = bottom as everywhere in the tests.
"""
from __future__ import annotations

import math

import numpy as np

from oracle import binding as O

CLAMP, REPEAT, MIXED = (False, False), (True, True), (True, False)
WRAPS = [CLAMP, REPEAT, MIXED]
TARGETS = [(4, np.uint8), (3, np.uint8), (4, np.float16), (4, np.float32)]          # (components, dtype) of a render target

# k_multipass_layer1's block and the blur's reach in uv units, multipass.frag:41 blur(iScreen0x0, astuv, 5, 8, 8):
# radius 5 times the last walk 7/8 over 2000 (every factor and the product exact in binary32's range of interest)
MP_BLOCK_W, MP_BLOCK_H = 64, 8
MP_REACH = 5.0*(7.0/8.0)/2000.0


def noise(seed, w: int, h: int, components: int = 4, dtype=np.uint8) -> np.ndarray:
    rng = seed if isinstance(seed, np.random.Generator) else np.random.default_rng(seed)
    data = rng.integers(0, 256, (h, w, components), dtype=np.uint8)
    return data if np.dtype(dtype) == np.uint8 else (data/255.0).astype(dtype)


def bits(a: np.ndarray) -> np.ndarray:
    """A render target as integers: float targets are compared on their bit patterns"""
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def wrap_id(wrap) -> str:
    return {CLAMP: "clamp", REPEAT: "repeat", MIXED: "repeat_x"}[tuple(wrap)]


def multipass_tile(w: int, h: int, lw: int, lh: int) -> tuple[int, int, int]:
    """launch_multipass_layer1's tile of a `w x h` target over a `lw x lh` layer: (texels wide, texels high, bytes of LDS)"""
    tile_w = math.ceil(MP_BLOCK_W*lw/w + 2.0*MP_REACH*lw) + 6
    tile_h = math.ceil(MP_BLOCK_H*lh/h + 2.0*MP_REACH*lh) + 6
    return tile_w, tile_h, tile_w*tile_h*16


def oracle_target(fragment: str, u, textures: dict, w: int, h: int, components: int = 4, dtype=np.uint8) -> np.ndarray:
    if components == 4 and np.dtype(dtype) == np.uint8:
        return O.render(fragment, u, textures, w, h, threads=8)
    return O.render_to(fragment, u, textures, w, h, components, dtype, threads=8)


def multipass_uniforms(w: int, h: int):
    return O.default_uniforms(w, h, iLayer=1)


def multipass_oracle(w, h, layer, background, wrap=CLAMP, filter="linear", components=4, dtype=np.uint8) -> np.ndarray:
    textures = {"background": O.make_texture(background), 0: O.make_texture(layer, filter, *wrap)}
    return oracle_target("multipass", multipass_uniforms(w, h), textures, w, h, components, dtype)


def motionblur_uniforms(w: int, h: int, temporal: int):
    u = O.default_uniforms(w, h, iLayer=1)
    u.user[0] = float(temporal)
    return u


def motionblur_oracle(w, h, layers, samplers, components=4, dtype=np.uint8) -> np.ndarray:
    """layers[t] with samplers[t] = (filter, repeat_x, repeat_y) is iScreen{t}x0"""
    textures = {t: O.make_texture(layers[t], *samplers[t]) for t in range(len(layers))}
    return oracle_target("motionblur", motionblur_uniforms(w, h, len(layers)), textures, w, h, components, dtype)


def fuzz_shape(rng: np.random.Generator):
    """w in [1, 320], h in [1, 96], a layer at 0.3 to 2.0 times the target per axis, wrap per axis, one of the four target types"""
    w, h = int(rng.integers(1, 321)), int(rng.integers(1, 97))
    lw = max(1, round(w*float(rng.uniform(0.3, 2.0))))
    lh = max(1, round(h*float(rng.uniform(0.3, 2.0))))
    wrap = (bool(rng.integers(0, 2)), bool(rng.integers(0, 2)))
    components, dtype = TARGETS[int(rng.integers(0, len(TARGETS)))]
    return w, h, lw, lh, wrap, components, dtype
