// The segment rule of an OpenDML AVI export (shaderflow_amd/mjpeg.py states the file; `segment_cuts` there is this rule in Python).
// Host only: no HIP include, so the rule can be compiled and checked alone (tests/ring_segments_check.cpp).
//
// The read-out ring's writer thread asks once per frame it writes: `run` is the bytes the frame puts into the file (its `00dc` chunk
// with the pad byte, and its `01wb` chunk with the pad byte when it has one). A RIFF chunk of the file spans at most `budget` bytes,
// unless one frame alone is larger; where the next frame would pass that, a gap of `gap` bytes goes in front of it and the next
// segment begins at the gap. A segment always takes at least one frame. All positions are 64-bit.
#pragma once
#include <cstdint>

struct RingSegments {
    uint64_t pos = 0;            // where the next byte of the file goes
    uint64_t seg_start = 0;      // where the current RIFF chunk begins (segment 0: byte 0, the headers count)
    uint64_t in_seg = 0;         // frames the current segment holds
    uint64_t budget = 0;         // bytes a RIFF chunk may span (0: no rule, never a gap)
    uint64_t gap = 0;            // bytes of a gap (`RIFF size AVIX LIST size movi`: 24)

    void begin(uint64_t start, uint64_t budget_, uint64_t gap_) { pos = start; seg_start = 0; in_seg = 0; budget = budget_; gap = gap_; }

    // The next written frame takes `run` bytes: does a gap go in front of it?
    bool cut(uint64_t run) {
        bool gap_first = false;
        if (budget && in_seg > 0 && pos + run - seg_start > budget) {
            seg_start = pos; pos += gap; in_seg = 0;
            gap_first = true;
        }
        pos += run; in_seg += 1;
        return gap_first;
    }
};
