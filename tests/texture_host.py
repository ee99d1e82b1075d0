"""
Test infrastructure: tests/jit_host.py's host build with a mip chain — `sfx_jit_host_texture_mips` (csrc/jit_runtime.hpp) attaches
levels 1 … and a mipmap filter to a texture already bound. The chain is the oracle's (`O.build_mipmaps`): its packing is glsl.hpp
mip_level's, every level 16-byte aligned (tests/test_host_texture.py checks the offsets).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from oracle import binding as O
from tests.jit_host import HostFragment

FILTERS = {"nearest": 0, "linear": 1, "linear_mipmap": 2, "nearest_mipmap": 3}      # csrc/glsl.hpp FILTER_*


def packed_offsets(width: int, height: int, texel_bytes: int, levels: int) -> list[int]:
    """byte offset of levels 1 … levels-1 as glsl.hpp mip_level walks them"""
    offsets, offset, w, h = [], 0, width, height
    for _ in range(1, levels):
        w, h = max(1, w >> 1), max(1, h >> 1)
        offsets.append(offset)
        offset += (w*h*texel_bytes + 15) & ~15
    return offsets


class TextureHostFragment(HostFragment):
    def bind_chain(self, name: str, data: np.ndarray, filter: str, repeat_x: bool, repeat_y: bool, *, mipmap: bool = True) -> O.Texture:
        """bind `data` with the chain the oracle builds from it; `mipmap`: the minification filter becomes the mipmap one (else the
        chain is attached under the plain filter). Returns the oracle's texture (levels through O.mip_level)."""
        assert self.bind(name, data, filter, repeat_x, repeat_y)
        texture = O.build_mipmaps(O.make_texture(self._keep[-1], filter, repeat_x, repeat_y))
        chain = np.concatenate([texture._chain, np.zeros(16, np.uint8)])      # (room for the device build's RGB8 over-read; unused on the host)
        self._keep.append(chain)
        binding = next(b for b in self.translation.bindings if b.name == name and b.sampler)
        code = FILTERS[f"{filter}_mipmap" if mipmap else filter]
        self.lib.sfx_jit_host_texture_mips(self.textures, binding.slot, chain.ctypes.data_as(C.c_void_p), texture.levels, code)
        return texture
