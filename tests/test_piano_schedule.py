"""
The host half of the piano sequence (shaderflow_amd/pianosequence.py) on the CPU: the note-range targets of all frames from one
vectorised pass equal what ShaderPiano.update() sets frame by frame, the grouping by pitch keeps the insertion order, the start-sorted
index is the visiting order of the notes that begin later, and the PianoRoll example's fragment translates and compiles for gfx950.
"""
import types
from pathlib import Path

import numpy as np
import pytest

from shaderflow_amd import glsl2hip as G
from shaderflow_amd.piano import PianoNote
from shaderflow_amd.piano.module import MAX_NOTE, ShaderPiano
from shaderflow_amd.pianosequence import group_by_pitch, note_range_targets, start_sorted, step_note_range

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = np.load(ROOT/"tests"/"golden"/"piano.npz")
CACHE = ROOT/"build"/"jit"


class Sink:
    def write(self, data=None, **kwargs):
        return self

    def clear(self):
        return self


def bare_piano(notes, **fields) -> ShaderPiano:
    """A ShaderPiano without a scene (as tests/test_host_piano.py builds one): fields at their defaults, textures that drop what is written"""
    piano = ShaderPiano.__new__(ShaderPiano)
    for attribute in ShaderPiano.__attrs_attrs__:
        default = attribute.default
        object.__setattr__(piano, attribute.name, default.factory() if hasattr(default, "factory") else default)
    for name, value in fields.items():
        setattr(piano, name, value)
    piano.scene = types.SimpleNamespace(time=0.0, dt=0.0, realtime=False)
    piano.keys_texture = piano.channel_texture = piano.roll_texture = piano.tempo_texture = Sink()
    for note in notes:
        piano.add_note(note)
    return piano


def golden_score():
    return [PianoNote(note=int(n), start=float(s), end=float(e), channel=int(c), velocity=int(v)) for n, s, e, c, v in GOLDEN["notes"]]


def random_score(seed=7, count=400):
    rng = np.random.default_rng(seed)
    notes = []
    for _ in range(count):
        start = float(rng.uniform(0.0, 12.0))
        # whole-second starts and ends, notes that end in the second they start in, and long ones
        start = float(np.floor(start)) if rng.random() < 0.2 else start
        notes.append(PianoNote(note=int(rng.integers(20, 110)), start=start, end=start + float(rng.choice([0.01, 0.2, 1.0, 3.5])),
                               channel=int(rng.integers(0, 4)), velocity=int(rng.integers(1, 128))))
    return notes


def clock(fps, frames, speed=1.0):
    times, dts, time, dt = [], [], 0.0, 0.0
    for _ in range(frames):
        times.append(time); dts.append(dt)
        dt = speed/fps
        time += dt
    return times, dts


@pytest.mark.parametrize("case", ["golden", "random", "random-offset", "empty"])
def test_vectorised_note_range_equals_update_frame_by_frame(case):
    notes = {"golden": golden_score, "random": random_score, "random-offset": random_score, "empty": list}[case]()
    fields = dict(time_offset=-1.75, roll_time=1.5, lookahead=0.75) if case == "random-offset" else {}
    fps, frames = (float(GOLDEN["fps"]), int(GOLDEN["frames"])) if case == "golden" else (24.0, 480)
    times, dts = clock(fps, frames)

    by_frame = bare_piano(notes, **fields)
    want_target, want_value = [], []
    for time, dt in zip(times, dts):
        by_frame.scene.time, by_frame.scene.dt = time, dt
        by_frame.update()
        want_target.append(by_frame.note_range_dynamics.target.copy())
        want_value.append(np.asarray(by_frame.note_range_dynamics.value, np.float32).copy())

    at_once = bare_piano(notes, **fields)
    shifted = [time + at_once.time_offset for time in times]
    # a small block: the pass over frames x notes is cut into several pieces
    lowest, highest, found = note_range_targets(at_once._table(), shifted, at_once.lookup_time, block=max(1, 7*len(notes)))
    for k in range(frames):
        pair = (lowest[k], highest[k]) if found[k] else (at_once.global_minimum_note, at_once.global_maximum_note)
        assert np.array_equal(np.asarray(pair, np.float32), want_target[k]), k
    if case != "empty":
        assert found.any() and (case == "golden" or not found.all())     # frames with and without candidates are both met
    values = step_note_range(at_once, times, dts)
    assert values.dtype == np.float32 and np.array_equal(values, np.asarray(want_value))
    if case == "golden":
        assert np.array_equal(values, GOLDEN["dynamic"])
    for name in ("value", "target", "previous", "derivative", "acceleration"):
        assert np.array_equal(getattr(at_once.note_range_dynamics, name), getattr(by_frame.note_range_dynamics, name)), name


def test_grouping_by_pitch_keeps_the_insertion_order():
    notes = random_score(seed=3, count=500)
    pitch = np.array([n.note for n in notes])
    first, order = group_by_pitch(pitch)
    assert first.shape == (MAX_NOTE + 1,) and first[0] == 0 and first[-1] == len(notes) and (np.diff(first) >= 0).all()
    assert sorted(order.tolist()) == list(range(len(notes)))
    for p in range(MAX_NOTE):
        members = order[first[p]:first[p + 1]]
        assert (pitch[members] == p).all() and (np.diff(members) > 0).all()
        assert members.tolist() == [k for k, n in enumerate(notes) if n.note == p]


def test_start_sorted_index_is_the_visiting_order_of_later_notes():
    """Far ahead of every note, all candidates of a pitch are 'later' ones: the reference's order is (starting second, insertion)"""
    notes = random_score(seed=5, count=300)
    piano = bare_piano(notes)
    table = piano._table()
    first, order = group_by_pitch(table["pitch"])
    by_start = start_sorted(first, table["start"][order])
    assert by_start.dtype == np.int32
    for p in range(MAX_NOTE):
        mine = by_start[first[p]:first[p + 1]]
        assert ((mine >= first[p]) & (mine < first[p + 1])).all()
        want = ShaderPiano._candidates(table, -5.0, 100.0, pitch=p)           # every note of the pitch, none begun
        assert order[mine].tolist() == want.tolist()


def test_piano_roll_fragment_translates_and_compiles_for_gfx950():
    from examples.scenes import PianoRoll
    defines = "".join(f"#define iPiano{name} iPiano{name}0x0\n" for name in ("Keys", "Chan", "Roll", "Tempo"))
    variables = [("sampler2D", f"iPiano{name}0x0") for name in ("Keys", "Chan", "Roll", "Tempo")]
    variables += [("int", "iPianoGlobalMin"), ("int", "iPianoGlobalMax"), ("vec2", "iPianoDynamic"), ("float", "iPianoRollTime"),
                  ("float", "iPianoExtra"), ("float", "iPianoHeight"), ("int", "iPianoLimit"), ("float", "iPianoBlackRatio")]
    translation = G.translate(defines + PianoRoll.FRAGMENT, variables)
    assert "SF_HD void main_()" in translation.cpp
    bound = {binding.name: binding for binding in translation.bindings}
    assert {"iPianoKeys0x0", "iPianoChan0x0", "iPianoRoll0x0", "iPianoDynamic", "iPianoRollTime", "iPianoExtra", "iPianoHeight",
            "iPianoLimit", "iPianoBlackRatio"} <= set(bound)
    assert bound["iPianoRoll0x0"].sampler and not bound["iPianoDynamic"].sampler and bound["iPianoDynamic"].count == 2
    assert bound["iPianoLimit"].integer and not bound["iPianoDynamic"].integer
    code = G.compile(translation, cache=CACHE)
    assert code.startswith((b"__CLANG_OFFLOAD_BUNDLE__", b"\x7fELF")) and b"gfx950" in code and b"sfx_jit_fused_2" in code
