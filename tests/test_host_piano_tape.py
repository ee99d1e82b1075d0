"""
The host halves of the piano-and-tape sequence that need no device: `clockloop.JoinedSource` with parts that record their calls, and
`synth.score_clip`, the sound of a score.
"""
from __future__ import annotations

import numpy as np
import pytest

from shaderflow_amd.clockloop import FrameSource, JoinedSource


class Part(FrameSource):
    """A frame source that writes every call into a shared log"""

    def __init__(self, name, log, shorten=None, settle_error=None, is_finished=True):
        self.name, self.log, self.shorten, self.settle_error, self.is_finished = name, log, shorten, settle_error, is_finished

    def prepare(self, times, dts, total): self.log.append((self.name, "prepare", total))
    def begin_batch(self, first, size): self.log.append((self.name, "begin_batch", first, size))
    def attach(self, sequence): self.log.append((self.name, "attach", sequence))
    def consumed(self, first, count): self.log.append((self.name, "consumed", first, count))
    def release(self): self.log.append((self.name, "release"))

    def take(self, sequence, first, count, batch_first):
        self.log.append((self.name, "take", first, count, batch_first))
        return count if self.shorten is None else min(count, self.shorten)

    def settle(self, done):
        self.log.append((self.name, "settle", done))
        if self.settle_error is not None:
            raise self.settle_error

    def finished(self, done, total):
        return self.is_finished


class Cutting(Part):
    def __init__(self, name, log, batch, **kwargs):
        super().__init__(name, log, **kwargs)
        self.batch = batch

    def batches(self, total):
        return [(first, min(self.batch, total - first)) for first in range(0, total, self.batch)]


def test_calls_reach_every_part_in_order():
    log = []
    joined = JoinedSource([Part("a", log), Cutting("b", log, 20), Part("c", log)], end="next", chunked=True)
    assert (joined.end, joined.chunked) == ("next", True)
    joined.prepare([0.0], [0.0], 45)
    joined.attach("descriptor")
    joined.begin_batch(20, 20)
    joined.consumed(20, 7)
    assert log == [("a", "prepare", 45), ("b", "prepare", 45), ("c", "prepare", 45),
                   ("a", "attach", "descriptor"), ("b", "attach", "descriptor"), ("c", "attach", "descriptor"),
                   ("a", "begin_batch", 20, 20), ("b", "begin_batch", 20, 20), ("c", "begin_batch", 20, 20),
                   ("a", "consumed", 20, 7), ("b", "consumed", 20, 7), ("c", "consumed", 20, 7)]


def test_end_and_chunked_default_to_the_plain_sources():
    joined = JoinedSource([Part("a", [])])
    assert (joined.end, joined.chunked) == (FrameSource.end, FrameSource.chunked)


def test_batches_come_from_the_part_that_cuts_the_run():
    log = []
    assert JoinedSource([Part("a", log), Cutting("b", log, 20)]).batches(45) == [(0, 20), (20, 20), (40, 5)]
    assert JoinedSource([Cutting("b", log, 30), Part("a", log)]).batches(45) == [(0, 30), (30, 15)]
    assert JoinedSource([Part("a", log), Part("c", log)]).batches(45) == [(0, 45)]
    with pytest.raises(ValueError, match="2 frame sources cut the run"):
        JoinedSource([Cutting("a", log, 20), Part("c", log), Cutting("b", log, 30)])


def test_take_threads_the_shortened_count_through():
    log = []
    joined = JoinedSource([Part("a", log), Part("b", log), Part("c", log, shorten=4)])
    assert joined.take("descriptor", 14, 7, 0) == 4
    assert log == [("a", "take", 14, 7, 0), ("b", "take", 14, 7, 0), ("c", "take", 14, 7, 0)]
    del log[:]
    assert joined.take("descriptor", 21, 3, 20) == 3                    # (nothing to shorten)
    assert [entry[3] for entry in log] == [3, 3, 3]


def test_a_part_that_shortens_a_call_must_be_the_last():
    log = []
    joined = JoinedSource([Part("a", log, shorten=4), Part("b", log)])
    with pytest.raises(AssertionError, match="shortened the call to 4 of 7"):
        joined.take("descriptor", 0, 7, 0)
    assert ("b", "take", 0, 4, 0) not in log and ("b", "take", 0, 7, 0) not in log
    assert joined.take("descriptor", 0, 4, 0) == 4                      # (a call it does not shorten is fine)


def test_settle_reaches_every_part_and_raises_the_first_error_again():
    log = []
    first, second = RuntimeError("first"), KeyError("second")
    joined = JoinedSource([Part("a", log, settle_error=first), Part("b", log), Part("c", log, settle_error=second)])
    with pytest.raises(RuntimeError) as raised:
        joined.settle(14)
    assert raised.value is first
    assert log == [("a", "settle", 14), ("b", "settle", 14), ("c", "settle", 14)]
    del log[:]
    JoinedSource([Part("a", log), Part("b", log)]).settle(3)            # (no error: none raised)
    assert log == [("a", "settle", 3), ("b", "settle", 3)]


def test_finished_is_the_conjunction_and_release_runs_in_reverse():
    log = []
    assert JoinedSource([Part("a", log), Part("b", log)]).finished(10, 10)
    assert not JoinedSource([Part("a", log), Part("b", log, is_finished=False)]).finished(10, 10)
    assert not JoinedSource([Part("a", log, is_finished=False), Part("b", log)]).finished(10, 10)
    JoinedSource([Part("a", log), Part("b", log), Part("c", log)]).release()
    assert log == [("c", "release"), ("b", "release"), ("a", "release")]


# ---- the sound of a score --------------------------------------------------------------------------------------------------------------

def score():
    from shaderflow_amd.piano import PianoNote
    return [PianoNote(note=33, start=0.5, end=1.0, channel=1, velocity=90), PianoNote(note=69, start=0.75, end=1.25, channel=0, velocity=100),
            PianoNote(note=96, start=1.5, end=2.0, channel=0, velocity=127)]


def test_score_clip_is_a_finite_stereo_float32_clip_inside_the_unit_range():
    from shaderflow_amd import synth
    clip = synth.score_clip(score(), 3.0, 22050)
    assert clip.shape == (66150, 2) and clip.dtype == np.float32
    assert np.isfinite(clip).all() and np.abs(clip).max() <= 1.0 and np.abs(clip).max() > 0.05
    assert synth.score_clip(score(), 2.0).shape == (88200, 2)            # 44 100 Hz unless said otherwise
    loud = synth.score_clip(score()*40, 3.0, 22050)                      # forty voices on every note: scaled, not clipped
    assert np.abs(loud).max() <= 1.0 and np.abs(loud).max() > 0.99


def test_score_clip_is_the_same_every_time():
    from shaderflow_amd import synth
    assert np.array_equal(synth.score_clip(score(), 3.0, 22050), synth.score_clip(score(), 3.0, 22050))


def test_score_clip_is_silent_where_the_score_is():
    from shaderflow_amd import synth
    rate = 22050
    clip = synth.score_clip(score(), 3.0, rate)
    at = lambda seconds: int(round(seconds*rate))
    assert not clip[:at(0.5)].any()                                       # before the first note
    assert clip[at(0.5):at(1.0)].any()
    assert not clip[at(1.25 + synth.SCORE_RELEASE) + 1:at(1.5)].any()    # between two notes, once the earlier one has faded
    assert clip[at(1.5):at(2.0)].any()
    assert not clip[at(2.0 + synth.SCORE_RELEASE) + 1:].any()            # after the last note's decay
    assert not synth.score_clip([], 1.0, rate).any()


def test_score_clip_pans_low_notes_left_and_high_notes_right():
    from shaderflow_amd import synth
    rate = 22050
    clip = synth.score_clip(score(), 3.0, rate)
    low, high = clip[int(0.55*rate):int(0.7*rate)], clip[int(1.55*rate):int(1.95*rate)]      # only note 33 sounds, only note 96 sounds
    assert np.abs(low[:, 0]).max() > 3*np.abs(low[:, 1]).max()
    assert np.abs(high[:, 1]).max() > 3*np.abs(high[:, 0]).max()
