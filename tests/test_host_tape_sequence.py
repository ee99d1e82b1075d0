"""
What the tape sequence (shaderflow_amd/tapesequence.py) needs of the translator, CPU only: a translated fragment says in its code object
whether it reads a uniform the tape sets per frame (sfx_jit_flags bit 1, csrc/jit_runtime.hpp SF_JIT_AUDIO).
"""
from __future__ import annotations

import pytest

from shaderflow_amd import glsl2hip as G


@pytest.mark.parametrize("name", sorted(G.AUDIO_UNIFORMS))
def test_fragments_reading_an_audio_uniform_are_marked(name):
    cpp = G.translate(f"void main() {{ fragColor = vec4({name}, stuv, 1.0); }}").cpp
    assert "#define SF_JIT_AUDIO 1" in cpp


def test_fragments_without_audio_uniforms_are_not_marked():
    assert "#define SF_JIT_AUDIO 0" in G.translate("void main() { fragColor = vec4(iTime, stuv, 1.0); }").cpp
    # (the samplers are told apart by their bindings: iSpectrogram and iWaveform have the slots the tape patches)
    translation = G.translate("void main() { fragColor = texture(iSpectrogram, astuv); }", [("sampler2D", "iSpectrogram")])
    assert "#define SF_JIT_AUDIO 0" in translation.cpp
    assert [(b.name, b.slot) for b in translation.bindings] == [("iSpectrogram", G.FIXED_SAMPLER_SLOTS["iSpectrogram"])]
