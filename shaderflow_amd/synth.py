"""
Deterministic synthetic inputs of the benchmark configurations: the reference's
own assets are downloaded from the network (examples/basic/demo.py:19-49) and are not available.
"""
from __future__ import annotations

import math

import numpy as np


def sweep_clip(seconds: float = 60.0, samplerate: int = 44100) -> np.ndarray:
    """(samples, 2) float32: L = 0.5*sin(phase) logarithmic sweep 20 Hz → 20 kHz, R = the same sweep reversed"""
    n = int(round(seconds*samplerate))
    t = np.arange(n, dtype=np.float64)/samplerate
    k = math.log(1000.0)
    phase = 2*math.pi*20.0*seconds/k*(np.exp(t/seconds*k) - 1.0)
    left = 0.5*np.sin(phase)
    return np.stack([left, left[::-1]], axis=1).astype(np.float32)


def background_image(width: int = 1920, height: int = 1080, seed: int = 0) -> np.ndarray:
    """(height, width, 3) uint8: low-frequency value noise over a gradient, top row first (an image file's order)"""
    rng = np.random.default_rng(seed)
    coarse = rng.random((height//40 + 2, width//40 + 2, 3))
    ys = np.linspace(0, coarse.shape[0] - 1.001, height)
    xs = np.linspace(0, coarse.shape[1] - 1.001, width)
    y0, x0 = ys.astype(int), xs.astype(int)
    fy, fx = (ys - y0)[:, None, None], (xs - x0)[None, :, None]
    noise = ((coarse[y0][:, x0]*(1 - fx) + coarse[y0][:, x0 + 1]*fx)*(1 - fy)
             + (coarse[y0 + 1][:, x0]*(1 - fx) + coarse[y0 + 1][:, x0 + 1]*fx)*fy)
    gradient = np.linspace(0.15, 0.85, width)[None, :, None]*np.array([0.9, 0.6, 1.0])[None, None, :]
    fine = rng.random((height, width, 3))*0.08
    return np.clip((0.55*noise + 0.45*gradient + fine)*255.0, 0, 255).astype(np.uint8)


SCORE_RELEASE = 0.05     # seconds a note of score_clip takes to fade to exact silence behind its end
SCORE_ATTACK = 0.005     # … and to rise in front (no click)


def score_clip(score, seconds: float, samplerate: int = 44100) -> np.ndarray:
    """(samples, 2) float32: the sound of a score (PianoNotes: note, start, end, velocity), so that a piano roll has audio that follows
    its notes without an asset. One sine per note at the pitch's equal-tempered frequency (A4 = note 69 = 440 Hz) from `start`, decaying
    as exp(-2 t) while the note is held and linearly to zero over SCORE_RELEASE behind `end`; constant-power panning, note 21 hard left
    to note 108 hard right; the sum is scaled down only if it would leave [-1, 1]. Silent wherever no note sounds."""
    n = int(round(seconds*samplerate))
    out = np.zeros((n, 2), np.float64)
    for note in score:
        first = max(0, int(math.ceil(note.start*samplerate)))
        last = min(n, int(math.floor((note.end + SCORE_RELEASE)*samplerate)) + 1)
        if last <= first:
            continue
        t = np.arange(first, last, dtype=np.float64)/samplerate - note.start
        held = note.end - note.start
        envelope = np.exp(-2.0*np.minimum(t, held))*np.clip(1.0 - (t - held)/SCORE_RELEASE, 0.0, 1.0)*np.clip(t/SCORE_ATTACK, 0.0, 1.0)
        tone = 0.35*(note.velocity/127.0)*envelope*np.sin(2*math.pi*440.0*2.0**((note.note - 69)/12.0)*t)
        pan = min(1.0, max(0.0, (note.note - 21)/87.0))*math.pi/2
        out[first:last, 0] += math.cos(pan)*tone
        out[first:last, 1] += math.sin(pan)*tone
    peak = float(np.abs(out).max()) if n else 0.0
    if peak > 1.0:
        out /= peak
    return out.astype(np.float32)
