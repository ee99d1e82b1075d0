"""
The reference's example scenes (examples/basic/demo.py:53-205) as they are written against its API — same class
names, same module construction, same parameters — with two differences forced by the environment:
fragments are named by their registry entry instead of a path into the reference's examples/basic/shaders/, and
assets are synthetic (shaderflow_amd.synth) because the originals are downloads (demo.py:16-49).
With the reference checked out, its own demo.py runs unchanged after `shaderflow_amd.install_alias()`.
`Plasma` is not from the reference: it shows a user-written fragment going through the run-time translator.
"""
from __future__ import annotations

import math
from pathlib import Path
from typing import Optional

import numpy as np

from shaderflow_amd import synth
from shaderflow_amd.dynamics import ShaderDynamics
from shaderflow_amd.scene import ShaderScene
from shaderflow_amd.shader import ShaderProgram
from shaderflow_amd.texture import ShaderTexture


class Basic(ShaderScene):
    """Simplest ShaderScene (demo.py:53-55): the built-in default fragment"""
    ...


class ShaderToy(ShaderScene):
    def build(self):
        self.shader.fragment = "shadertoy"


class MultiShader(ShaderScene):
    """Two shaders acting together (demo.py:67-89)"""
    def build(self):
        self.child = ShaderProgram(scene=self, name="child")
        self.child.fragment = "multi_child"
        self.shader.fragment = "multi_main"


class Dynamics(ShaderScene):
    """Second order system driven from python every frame (demo.py:114-129): frame-loop only"""
    background: Optional[np.ndarray] = None

    def build(self):
        image = self.background if self.background is not None else synth.background_image(480, 270)
        ShaderTexture(scene=self, name="background").from_numpy(image)
        self.dynamics = ShaderDynamics(scene=self, name="iShaderDynamics", frequency=4)
        self.shader.fragment = "dynamics"

    def update(self):
        self.dynamics.target = 0.5*(1 + np.sign(np.sin(2*math.pi*self.time*0.5)))


class _AudioScene(ShaderScene):
    """Scenes below take `audio=` as a WAV path or a (samples (n, channels) float32, samplerate) pair"""
    audio_source = None

    def _load_audio(self):
        from shaderflow_amd.audio import ShaderAudio
        self.audio = ShaderAudio(scene=self, name="iAudio")
        source = self.audio_source
        if isinstance(source, (str, Path)):
            self.audio.file = source
        elif source is not None:
            samples, samplerate = source
            self.audio.load(samples=samples, samplerate=samplerate)


class Waveform(_AudioScene):
    """Audio waveform oscilloscope (demo.py:157-166)"""
    def build(self):
        from shaderflow_amd.audio.waveform import ShaderWaveform
        self._load_audio()
        self.waveform = ShaderWaveform(scene=self, audio=self.audio, smooth=False)
        self.shader.fragment = "waveform"


class MusicBars(_AudioScene):
    """Basic music bars (demo.py:170-184)"""
    def build(self):
        from shaderflow_amd.audio.spectrogram import ShaderSpectrogram
        from shaderflow_amd.piano import PianoNote
        self._load_audio()
        self.spectrogram = ShaderSpectrogram(scene=self, audio=self.audio, length=0)
        self.spectrogram.from_notes(start=PianoNote.from_frequency(20), end=PianoNote.from_frequency(18000), piano=True)
        self.shader.fragment = "bars"


class Visualizer(_AudioScene):
    """Radial bars music visualizer (demo.py:188-205) — the benchmark scene"""
    background: Optional[np.ndarray] = None

    def build(self):
        from shaderflow_amd.audio.spectrogram import ShaderSpectrogram
        from shaderflow_amd.audio.waveform import ShaderWaveform
        from shaderflow_amd.piano import PianoNote
        self._load_audio()
        self.waveform = ShaderWaveform(scene=self, audio=self.audio)
        self.spectrogram = ShaderSpectrogram(scene=self, length=0, audio=self.audio, smooth=False)
        self.spectrogram.from_notes(start=PianoNote.from_frequency(20), end=PianoNote.from_frequency(14000), piano=True)
        image = self.background if self.background is not None else synth.background_image(1920, 1080)
        self.back = ShaderTexture(scene=self, name="background").from_numpy(image)
        self.shader.fragment = "visualizer"


class Multipass(ShaderScene):
    """Multi layers done on a single shader (demo.py:93-99)"""
    background: Optional[np.ndarray] = None

    def build(self):
        image = self.background if self.background is not None else synth.background_image(480, 270)
        ShaderTexture(scene=self, name="background").from_numpy(image)
        self.shader.texture.layers = 2
        self.shader.fragment = "multipass"


class MotionBlur(ShaderScene):
    """Poor's man Motion Blur (demo.py:103-110)"""
    background: Optional[np.ndarray] = None

    def build(self):
        image = self.background if self.background is not None else synth.background_image(480, 270)
        ShaderTexture(scene=self, name="background").from_numpy(image)
        self.shader.texture.temporal = 10
        self.shader.texture.layers = 2
        self.shader.fragment = "motionblur"


class RayMarch(ShaderScene):
    """Ray Marching demo (demo.py:215-219)"""
    def build(self):
        self.shader.fragment = "raymarch"


class Life(ShaderScene):
    """Conway's Game of Life on the GPU (demo.py:223-247): a float simulation texture with ten frames of history"""
    life_period: int = 6
    shard_warmup = None                  # every generation depends on all earlier ones: a shard renders from frame 0

    def setup(self):
        width, height = 192, 108
        random = np.random.randint(0, 2, (width, height), dtype=bool)
        self.simulation.texture.size = (width, height)
        self.simulation.texture.write(random.astype(np.float32), temporal=1)

    def build(self):
        self.simulation = ShaderProgram(scene=self, name="iLife")
        self.simulation.texture.temporal = 10
        self.simulation.texture.filter = "nearest"
        self.simulation.texture.dtype = "f4"
        self.simulation.texture.components = 1
        self.simulation.texture.track = False
        self.simulation.fragment = "life_simulation"
        self.shader.fragment = "life_visuals"

    def pipeline(self):
        from shaderflow_amd.variable import Uniform
        yield from ShaderScene.pipeline(self)
        yield Uniform("int", "iLifePeriod", self.life_period)


class Mandelbrot(ShaderScene):
    """Mandelbrot fractal (examples/fractals/fractals.py:7-10)"""
    def build(self):
        self.shader.fragment = "mandelbrot"


class Tetration(ShaderScene):
    """Complex tetration fractal (examples/fractals/fractals.py:12-15)"""
    def build(self):
        self.shader.fragment = "tetration"


class Video(ShaderScene):
    """Video as a texture (shaderflow/video.py + examples/basic/shaders/video.frag; demo.py has no scene for it):
    `clip` = (frames (n, h, w, 3) uint8, fps) or a path: a `.npy` of such frames, a `.y4m` file (YUV4MPEG2, 8-bit progressive 4:2:0, read
    natively: size and rate come from its header), or any container an ffmpeg binary on PATH decodes. Raw `.rgb` and raw planar `.yuv` /
    `.i420` files carry no size: give them to a ShaderVideo of your own with `width=`, `height=` and `fps=` (shaderflow_amd/video.py).
    Without python logic of its own the scene is drawn by the video sequence (shaderflow_amd/videosequence.py)."""
    clip = None

    def build(self):
        from shaderflow_amd.video import ShaderVideo
        if isinstance(self.clip, (str, Path)):
            self.video = ShaderVideo(scene=self, path=self.clip)
        else:
            frames, fps = self.clip if self.clip is not None else (synth.background_image(64, 36)[None].repeat(4, 0), 30.0)
            self.video = ShaderVideo(scene=self, frames=frames, fps=fps)
        self.shader.fragment = "video"


class Plasma(ShaderScene):
    """A scene with a fragment of its own (not one of the reference's): the GLSL below is translated to HIP C++, compiled
    with hipcc on first use and cached (shaderflow_amd/glsl2hip.py). Scene-defined uniforms come from `pipeline()` like in the
    reference; being a stock scene otherwise, it batches through the clock tape."""
    FRAGMENT = """
        // sum of rotating plane waves, coloured through the prelude's hsv2rgb
        #define WAVES 5
        float wave(vec2 p, float k) {
            vec2 direction = vec2(cos(k*1.3), sin(k*1.3));
            return sin(dot(direction, p)*(3.0 + k) + iTime*(0.6 + 0.2*k));
        }
        void main() {
            GetCamera(iCamera);
            vec2 p = iCamera.gluv*rotate2d(0.1*iTime);
            float sum = 0;
            for (int k = 0; k < WAVES; k++)
                sum += wave(p, float(k))/WAVES;
            vec3 colour = hsv2rgb(vec3(TAU*fract(0.5*sum + 0.05*iTime), 0.75, 0.6 + 0.4*sum));
            colour *= 1 - 0.3*smoothstep(0.5, 1.5, length(iCamera.gluv));
            fragColor = vec4(colour, 1);
        }
    """

    def build(self):
        super().build()
        self.shader.fragment = self.FRAGMENT


class Bloom(ShaderScene):
    """A picture with a glow: a fragment of its own that gathers the bright parts around every pixel with a loop of taps — the kind
    of fragment whose sampler the kernels serve from an LDS tile (DESIGN.md §9 "Translated fragments"; `SHADERFLOW_JIT_TILE=0`
    renders the same frames without it)"""
    background: Optional[np.ndarray] = None
    FRAGMENT = """
        uniform float iGlow = 0.6;
        void main() {
            vec2 texel = 1.0/vec2(textureSize(background, 0));
            float reach = 2.0 + 1.5*sin(iTime);
            vec3 glow = vec3(0);
            float total = 0;
            for (int x = -4; x <= 4; x++) {
                for (int y = -4; y <= 4; y++) {
                    float weight = exp(-float(x*x + y*y)/8.0);
                    vec3 tap = texture(background, astuv + vec2(x, y)*texel*reach).rgb;
                    glow += weight*max(tap - 0.5, 0.0);
                    total += weight;
                }
            }
            fragColor = vec4(texture(background, astuv).rgb + iGlow*2.0*glow/total, 1);
        }
    """

    def build(self):
        super().build()
        image = self.background if self.background is not None else synth.background_image(640, 360)
        self.back = ShaderTexture(scene=self, name="background").from_numpy(image)
        self.shader.fragment = self.FRAGMENT


class Glow(ShaderScene):
    """The cheap glow of Shadertoy-style fragments: the picture's own mip chain is the blur. `mipmaps=True` builds the chain on the
    device, `textureLod(background, uv, k)` reads level k — each a picture blurred twice as wide as the one before — and the bright
    parts of levels 1 … 5 are summed over the image. The image itself is softened by a 3 x 3 box of `textureOffset` taps (whole
    texels of the level the lookup selects — here, under a chain, the level the pixel's own footprint asks for; the loop of taps
    earns the sampler an LDS tile, which a mipmapped texture bypasses: the draw takes the code object's untiled twin)."""
    background: Optional[np.ndarray] = None
    FRAGMENT = """
        uniform float iGlow = 0.7;
        void main() {
            vec3 image = vec3(0);
            for (int x = -1; x <= 1; x++)
                for (int y = -1; y <= 1; y++)
                    image += textureOffset(background, astuv, ivec2(x, y)).rgb/9.0;
            vec3 glow = vec3(0);
            for (int k = 1; k <= 5; k++)
                glow += max(textureLod(background, astuv, float(k)).rgb - 0.45, 0.0)/5.0;
            fragColor = vec4(image + iGlow*(1.5 + sin(iTime))*glow, 1);
        }
    """

    def build(self):
        super().build()
        image = self.background if self.background is not None else synth.background_image(640, 360)
        self.back = ShaderTexture(scene=self, name="background", mipmaps=True).from_numpy(image)
        self.back.repeat(True)                                        # applies the sampler state: builds the chain of the picture
        self.shader.fragment = self.FRAGMENT


class AudioTrails(_AudioScene):
    """Audio-reactive trails (not one of the reference's): a fragment of its own, translated at run time, with two layers and four
    frames of history. Layer 0 draws the spectrum as a ring of bars around a disc that breathes with the volume; layer 1 lays it over
    its own previous frame, zoomed in a little and faded, so every bar leaves a trail — the kind of feedback scene a user of the
    Visualizer writes next. No python logic between frames: it renders on the device audio tape (shaderflow_amd/tapesequence.py)."""
    FRAGMENT = """
        void main() {
            if (iLayer == 0) {
                float angle = abs(atan(gluv.y, gluv.x))/PI;
                vec2 s = texture(iSpectrogram, vec2(0.5, angle)).xy;
                float bar = 0.5*sqrt(max(0.5*(s.x + s.y), 0.0)/1000.0);
                float radius = 0.25 + 0.15*iAudioVolume;
                float r = length(gluv);
                float ring = smoothstep(radius - 0.01, radius, r)*(1.0 - smoothstep(radius + bar, radius + bar + 0.01, r));
                vec3 colour = hsv2rgb(vec3(fract(angle*0.5 + 0.1*iTime), 0.7, 1.0))*ring;
                colour += vec3(0.1, 0.15, 0.3)*(1.0 - smoothstep(0.0, radius, r))*(0.5 + iAudioVolume);
                fragColor = vec4(colour, 1.0);
                return;
            }
            vec4 now = texture(iScreen0x0, astuv);
            vec2 inward = 0.5 + (astuv - 0.5)*(0.98 - 0.02*iAudioVolume);
            vec3 trail = 0.6*iScreenTexture(1, 1, inward).rgb + 0.3*iScreenTexture(3, 1, inward).rgb;
            fragColor = vec4(max(now.rgb, trail), 1.0);
        }
    """

    def build(self):
        from shaderflow_amd.audio.spectrogram import ShaderSpectrogram
        from shaderflow_amd.piano import PianoNote
        self._load_audio()
        self.spectrogram = ShaderSpectrogram(scene=self, length=0, audio=self.audio, smooth=False)
        self.spectrogram.from_notes(start=PianoNote.from_frequency(20), end=PianoNote.from_frequency(14000), piano=True)
        self.shader.texture.temporal = 4
        self.shader.texture.layers = 2
        self.shader.fragment = self.FRAGMENT

def demo_score(seconds: float = 8.0) -> list:
    """A few bars for PianoRoll: a bass note per bar on channel 1 under broken chords on channel 0"""
    from shaderflow_amd.piano import PianoNote
    chords = ((48, 55, 60, 64, 67), (45, 52, 57, 60, 64), (41, 48, 53, 57, 60), (43, 50, 55, 59, 62))
    notes, bar = [], 0
    while 2.0*bar < seconds:
        start, chord = 2.0*bar, chords[bar % 4]
        notes.append(PianoNote(note=chord[0] - 12, start=start, end=start + 1.9, channel=1, velocity=70))
        for k in range(8):
            pitch = chord[1 + (3*k) % 4] + (12 if k % 4 == 3 else 0)
            notes.append(PianoNote(note=pitch, start=start + 0.25*k, end=start + 0.25*k + 0.22, channel=0, velocity=60 + 10*(k % 4)))
        bar += 1
    return notes


class PianoRoll(ShaderScene):
    """A piano roll (not one of the reference's, which ships the module without a scene): a keyboard strip whose keys light up in the
    colour of the channel that plays them, and above it the notes of the next `roll_time` seconds falling onto the keys. The fragment
    reads what ShaderPiano exports: iPianoKeys / iPianoChan per key, iPianoRoll per (slot, pitch), the note range iPianoDynamic.
    `score`: PianoNotes, or the path of a MIDI file. No python logic between frames: the score lives on the device and the frames come
    from the native piano sequence (shaderflow_amd/pianosequence.py)."""
    score = None
    FRAGMENT = """
        bool blackKey(int note) {
            int k = note % 12;
            return k == 1 || k == 3 || k == 6 || k == 8 || k == 10;
        }
        vec3 channelColour(float channel) {
            return 0.55 + 0.45*cos(TAU*(0.19*channel + vec3(0.0, 0.33, 0.67)));
        }
        void main() {
            // the keys on screen: the note range the module follows, and a margin on both sides
            float low = iPianoDynamic.x - iPianoExtra;
            float high = iPianoDynamic.y + iPianoExtra + 1.0;
            float key = mix(low, high, astuv.x);
            int note = int(floor(key));
            float across = fract(key);
            vec3 colour = vec3(0.05, 0.05, 0.08);
            if (note < 0 || note > 127) {
                fragColor = vec4(colour, 1.0);
                return;
            }
            bool black = blackKey(note);
            float gap = smoothstep(0.0, 0.08, across)*smoothstep(0.0, 0.08, 1.0 - across);
            if (astuv.y < iPianoHeight) {
                // the keyboard strip: a black key covers the upper part of its column
                float up = astuv.y/iPianoHeight;
                float pressed = clamp(texelFetch(iPianoKeys, ivec2(note, 0), 0).x/100.0, 0.0, 1.0);
                float channel = texelFetch(iPianoChan, ivec2(note, 0), 0).x;
                bool dark = black && up > 1.0 - iPianoBlackRatio;
                vec3 rest = dark ? vec3(0.07) : vec3(0.9);
                vec3 lit = channel < 0.0 ? rest : channelColour(channel);
                colour = mix(rest, lit, pressed)*mix(0.55, 1.0, gap)*(0.8 + 0.2*up);
            } else {
                // the roll: height above the strip is time ahead of now
                float when = iTime + iPianoRollTime*(astuv.y - iPianoHeight)/(1.0 - iPianoHeight);
                colour += black ? vec3(0.0) : vec3(0.025);
                for (int slot = 0; slot < iPianoLimit; slot++) {
                    vec4 entry = texelFetch(iPianoRoll, ivec2(slot, note), 0);
                    if (entry.y == 0.0 && entry.w == 0.0)
                        break;
                    if (when >= entry.x && when <= entry.y)
                        colour = channelColour(entry.z)*(0.45 + 0.55*entry.w/127.0)*mix(0.3, 1.0, gap);
                }
            }
            fragColor = vec4(colour, 1.0);
        }
    """

    def build(self):
        from shaderflow_amd.piano import ShaderPiano
        super().build()
        self.piano = ShaderPiano(scene=self)
        score = demo_score() if self.score is None else self.score
        if isinstance(score, (str, Path)):
            self.piano.load_midi(score)
        else:
            for note in score:
                self.piano.add_note(note)
        self.shader.fragment = self.FRAGMENT


class PianoAudio(_AudioScene):
    """A piano roll with its sound track (not one of the reference's): PianoRoll's keyboard and falling notes, and under the keyboard
    a spectrum strip — one bin of iSpectrogram per key, drawn in the key's column — while the keys glow with iAudioVolume. `score` as
    for PianoRoll; `audio` as for the audio scenes, and without one the score's own sound (synth.score_clip). No python logic between
    frames: the piano and the audio tape feed one native sequence (shaderflow_amd/sequence.py)."""
    score = None
    SPECTRUM_LOW, SPECTRUM_HIGH = 21, 108                           # A0 … C8: one spectrogram bin per key of an 88-key piano
    FRAGMENT = """
        #define SPECTRUM_LOW 21.0
        #define SPECTRUM_KEYS 88.0
        bool blackKey(int note) {
            int k = note % 12;
            return k == 1 || k == 3 || k == 6 || k == 8 || k == 10;
        }
        vec3 channelColour(float channel) {
            return 0.55 + 0.45*cos(TAU*(0.19*channel + vec3(0.0, 0.33, 0.67)));
        }
        void main() {
            // the keys on screen: the note range the module follows, and a margin on both sides
            float low = iPianoDynamic.x - iPianoExtra;
            float high = iPianoDynamic.y + iPianoExtra + 1.0;
            float key = mix(low, high, astuv.x);
            int note = int(floor(key));
            float across = fract(key);
            vec3 colour = vec3(0.05, 0.05, 0.08);
            if (note < 0 || note > 127) {
                fragColor = vec4(colour, 1.0);
                return;
            }
            bool black = blackKey(note);
            float gap = smoothstep(0.0, 0.08, across)*smoothstep(0.0, 0.08, 1.0 - across);
            float strip = 0.25*iPianoHeight;
            if (astuv.y < strip) {
                // the spectrum strip: the level of the key's own bin, both channels, rising from the bottom edge
                vec2 s = texture(iSpectrogram, vec2(0.5, (key - SPECTRUM_LOW)/SPECTRUM_KEYS)).xy;
                float level = clamp(sqrt(max(0.5*(s.x + s.y), 0.0))/30.0, 0.0, 1.0);
                float up = astuv.y/strip;
                vec3 bar = hsv2rgb(vec3(0.66 - 0.6*level, 0.8, 1.0))*mix(0.5, 1.0, gap);
                colour = mix(colour, bar, step(up, level));
            } else if (astuv.y < iPianoHeight) {
                // the keyboard: a black key covers the upper part of its column; a key that is down glows with the loudness of the moment
                float up = (astuv.y - strip)/(iPianoHeight - strip);
                float pressed = clamp(texelFetch(iPianoKeys, ivec2(note, 0), 0).x/100.0, 0.0, 1.0);
                float channel = texelFetch(iPianoChan, ivec2(note, 0), 0).x;
                bool dark = black && up > 1.0 - iPianoBlackRatio;
                vec3 rest = dark ? vec3(0.07) : vec3(0.9);
                vec3 lit = channel < 0.0 ? rest : channelColour(channel);
                colour = mix(rest, lit, pressed)*mix(0.55, 1.0, gap)*(0.8 + 0.2*up);
                colour += 0.6*lit*pressed*clamp(iAudioVolume, 0.0, 1.0)*up;
            } else {
                // the roll: height above the keyboard is time ahead of now
                float when = iTime + iPianoRollTime*(astuv.y - iPianoHeight)/(1.0 - iPianoHeight);
                colour += black ? vec3(0.0) : vec3(0.025);
                for (int slot = 0; slot < iPianoLimit; slot++) {
                    vec4 entry = texelFetch(iPianoRoll, ivec2(slot, note), 0);
                    if (entry.y == 0.0 && entry.w == 0.0)
                        break;
                    if (when >= entry.x && when <= entry.y)
                        colour = channelColour(entry.z)*(0.45 + 0.55*entry.w/127.0)*mix(0.3, 1.0, gap);
                }
            }
            fragColor = vec4(colour, 1.0);
        }
    """

    def build(self):
        from shaderflow_amd.audio.spectrogram import ShaderSpectrogram
        from shaderflow_amd.piano import ShaderPiano
        super().build()
        self.piano = ShaderPiano(scene=self)
        score = demo_score() if self.score is None else self.score
        if isinstance(score, (str, Path)):
            self.piano.load_midi(score)
        else:
            for note in score:
                self.piano.add_note(note)
        if self.audio_source is None:
            self.audio_source = (synth.score_clip(list(self.piano.notes), self.piano.duration + 1.0), 44100)
        self._load_audio()
        self.spectrogram = ShaderSpectrogram(scene=self, length=0, audio=self.audio, smooth=False)
        self.spectrogram.from_notes(start=self.SPECTRUM_LOW, end=self.SPECTRUM_HIGH, piano=True)
        self.shader.fragment = self.FRAGMENT


def drifting_clip(width: int = 320, height: int = 180, step: int = 3):
    """An endless clip for MusicVideo: synth.background_image drifting to the right by `step` pixels a frame, (height, width, 3) uint8"""
    import itertools
    image = synth.background_image(width, height, seed=3)
    return (np.roll(image, step*k, axis=1) for k in itertools.count())


class MusicVideo(_AudioScene):
    """A clip with its sound track (not one of the reference's): the video fills the frame and glows with iAudioVolume, and along the
    bottom edge runs a spectrum strip, one bin of iSpectrogram per column. `clip` as for Video — (frames, fps), or a path: a `.npy`, a
    `.y4m` file, or what an ffmpeg binary decodes — and without one a drifting synthetic picture at 30 frames a second; `audio` as for
    the audio scenes, and without one a sine sweep. No python logic between frames: the staged video and the audio tape feed one
    native sequence (shaderflow_amd/sequence.py)."""
    clip = None
    CLIP_SIZE, CLIP_FPS = (320, 180), 30.0
    FRAGMENT = """
        #define STRIP 0.2
        void main() {
            vec3 colour = texture(iVideo, astuv).rgb;
            float loud = clamp(iAudioVolume, 0.0, 1.0);
            // the glow: the picture brightens with the loudness of the moment, most towards the edges
            colour = colour*(0.75 + 0.5*loud) + vec3(0.25, 0.12, 0.35)*loud*smoothstep(0.4, 1.4, length(gluv));
            if (astuv.y < STRIP) {
                // the spectrum strip: the level of the column's bin, both channels, rising from the bottom edge over the dimmed clip
                vec2 s = texture(iSpectrogram, vec2(0.5, astuv.x)).xy;
                float level = clamp(sqrt(max(0.5*(s.x + s.y), 0.0))/30.0, 0.0, 1.0);
                float up = astuv.y/STRIP;
                vec3 bar = hsv2rgb(vec3(0.66 - 0.6*level, 0.8, 1.0))*(0.6 + 0.4*up);
                colour = mix(0.45*colour, bar, step(up, level));
            }
            fragColor = vec4(colour, 1.0);
        }
    """

    def build(self):
        from shaderflow_amd.audio.spectrogram import ShaderSpectrogram
        from shaderflow_amd.piano import PianoNote
        from shaderflow_amd.video import ShaderVideo
        super().build()
        if isinstance(self.clip, (str, Path)):
            self.video = ShaderVideo(scene=self, path=self.clip)
        elif self.clip is not None:
            frames, fps = self.clip
            self.video = ShaderVideo(scene=self, frames=frames, fps=fps)
        else:
            (width, height), fps = self.CLIP_SIZE, self.CLIP_FPS
            self.video = ShaderVideo(scene=self, frames=drifting_clip(width, height), width=width, height=height, fps=fps)
        if self.audio_source is None:
            self.audio_source = (synth.sweep_clip(10.0, 44100), 44100)
        self._load_audio()
        self.spectrogram = ShaderSpectrogram(scene=self, length=0, audio=self.audio, smooth=False)
        self.spectrogram.from_notes(start=PianoNote.from_frequency(20), end=PianoNote.from_frequency(14000), piano=True)
        self.shader.fragment = self.FRAGMENT


def make(cls, audio=None, background=None, score=None, clip=None, **fields):
    """Build a scene class with its inputs set before `build()` runs (class attributes, like demo.py's Life)"""
    attrs = {}
    if clip is not None:
        attrs["clip"] = clip
    if score is not None:
        attrs["score"] = score
    if audio is not None:
        attrs["audio_source"] = audio
    if background is not None:
        attrs["background"] = background
    return type(cls.__name__, (cls,), attrs)(**fields)
