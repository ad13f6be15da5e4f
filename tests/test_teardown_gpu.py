"""Teardown (run with -m gpu on an MI355X): a context's device buffers, events, streams and pinned blocks go with it --
no member of crt_ctx has a line in crt_destroy -- and a stream adopted through crt_set_stream does not."""
import pytest

pytestmark = pytest.mark.gpu


def _lost_between_cycle_5_and_25(samples):
    """Free device memory after cycle 5 minus after cycle 25 of create -> upload -> build -> frame(samples) -> close, no sync."""
    import torch
    from computeraytracer_amd import Renderer, cornell
    ps = cornell(96, 64)
    torch.cuda.synchronize()
    free = {}
    for k in range(1, 26):
        r = Renderer(0)
        r.upload(ps).build_accel("bvh2").frame(samples)          # no sync: close() finds the call as it was left
        r.close()
        free[k] = torch.cuda.mem_get_info(0)[0]
    print(f"frame({samples}): free device memory after cycle 5 minus after cycle 25: {free[5] - free[25]} bytes")
    return free[5] - free[25]


# Measured once on an MI355X with the same loop (the runtime may keep pools of its own, so the bound is the parent
# commit's figure, not a derived one):
#   frame(2)   a small call that is only noted (it waits to be merged with the next ones): parent 0 bytes, this commit 0 bytes
#   frame(32)  two cohorts' worth: the batch is published and the pool is at work when close() comes: parent 0 bytes, this commit 0 bytes
# (free memory was the same after every one of the 25 cycles, at both commits, for both loops)
@pytest.mark.parametrize("samples,parent_lost", [(2, 0), (32, 0)])
def test_contexts_leave_no_device_memory_behind(samples, parent_lost):
    assert _lost_between_cycle_5_and_25(samples) <= parent_lost


def test_adopted_stream_survives_close():
    """A stream adopted through crt_set_stream is the caller's: close() drains it and leaves it alone."""
    import torch
    from computeraytracer_amd import Renderer, cornell
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    r = Renderer(0)
    r.upload(cornell(96, 64)).build_accel("bvh2")
    r.set_stream(stream.cuda_stream)
    r.frame(2)
    r.close()
    with torch.cuda.stream(stream):
        t = torch.arange(4096, dtype=torch.int64, device=dev) * 3
    stream.synchronize()
    assert int(t.sum().item()) == 3 * 4095 * 4096 // 2
