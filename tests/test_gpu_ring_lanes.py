"""
The read-out ring's copier over its lane counts (csrc/capi_readout.hip ring_copier, the loop of csrc/lane_pump.hpp): eleven odd-sized
frames through rings of 1, 2, 3 and 5 slots — 1, 1, 2 and 4 lanes, every slot and lane used more than twice — into a file, on the
default route and on HIP's copy streams.
"""
import ctypes as C

import numpy as np
import pytest

from shaderflow_amd import _native as N

pytestmark = pytest.mark.gpu

FRAMES, FRAME_BYTES, STRIDE = 11, 4099, 4112


@pytest.mark.parametrize("route", ["default", "hip"])
@pytest.mark.parametrize("slots", [1, 2, 3, 5])
def test_frames_arrive_in_order_for_every_lane_count(slots, route, tmp_path, monkeypatch):
    """The file holds the frames in order, byte for byte (4 099 bytes: 16-byte words and a tail of 3)"""
    import torch
    if route == "hip":
        monkeypatch.setenv("SHADERFLOW_READOUT", "hip")
    else:
        monkeypatch.delenv("SHADERFLOW_READOUT", raising=False)
    rng = np.random.default_rng(100*slots)
    frames = np.zeros((FRAMES, STRIDE), np.uint8)
    for k in range(FRAMES):
        frames[k, :FRAME_BYTES] = (rng.integers(0, 256, FRAME_BYTES) + 23*k) % 251      # its own pattern per frame
    context = N.Context(N.default_context().device)                     # the route is read once per context: a fresh one
    ring = N.Handle()
    try:
        N.check(N.lib().sfx_ring_create(context.handle, FRAME_BYTES, slots, C.byref(ring)))
        try:
            device = torch.from_numpy(frames).cuda()
            torch.cuda.synchronize()
            with open(tmp_path/"out.bin", "wb") as file:
                N.check(N.lib().sfx_ring_pipe_frames(ring, C.c_void_p(device.data_ptr()), STRIDE, FRAMES, 0, -1, file.fileno()))
                N.check(N.lib().sfx_ring_pipe_sync(ring, -1))
        finally:
            N.check(N.lib().sfx_ring_destroy(ring))
    finally:
        context.destroy()
    got = np.frombuffer((tmp_path/"out.bin").read_bytes(), np.uint8)
    assert got.size == FRAMES*FRAME_BYTES
    assert np.array_equal(got.reshape(FRAMES, FRAME_BYTES), frames[:, :FRAME_BYTES])
