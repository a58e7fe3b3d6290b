"""The weight-gradient side stream: the one place where it becomes current and the one place
where the buffers it uses are held.

Work off the backward's critical path (in_backward -> input gradient -> ...) runs on a second
HIP stream beside it: the weight gradients, their slice reductions, the heads' weight
gradients, the loss values, the weight packing and the noise draw.  Every device has one lane:
its side stream and the list of buffers that stream is using (None: idle since the last join).
The lifetime rule:
* The side stream becomes current only inside run().  On entry it waits for the caller's
  stream (its inputs are ready), the lane becomes pending and holds the block's inputs;
  keep(...) adds what the block allocates.  The caller's stream waits for the side stream
  once, at join() -- at the end of a batched_wgrad_reduce() block, or inside
  deferred_side_join() (the trainer's backward) only when that block exits -- and only then is
  the list dropped: any later use of those blocks is ordered behind that wait.  They are held
  on the host, not through record_stream: its event records on every free cost the GPU idle
  time at each join.
* Blocks allocated inside run() belong to the side stream's allocator pool and are its to
  reuse once freed, while the caller's stream may still be reading them: the `on_main` final
  flush (engine.batched_wgrad_reduce) sums the side stream's partials on the caller's stream
  after the join and frees them without record_stream.  That is safe because the first entry
  after a join always forks (resume=True needs a pending lane): the side stream first waits on
  a point of the caller's stream at or after every launch issued before the entry.
* A kernel-attached fork (fork= a fork_arm() token) waits on the armed InstanceNorm-backward
  apply launch only, not on an event recorded at the entry, and it can be the first entry
  after a join (the encoder backward under autograd).  That is still late enough.  The caller
  launches nothing between the apply and the entry, so the apply is the last writer of what
  the block reads.  And the apply is launched after fork_arm(), behind everything the caller's
  stream was given before the arm -- the readers of freed blocks among it, because the final
  flush is issued, and its partials freed, before its batched_wgrad_reduce() block returns.
The lanes are per process: forward and autograd-backward threads share them.
"""
import contextlib
import ctypes
import functools
import os

import torch

from . import _native as N

# EBSDVAE_WGRAD_STREAM=0 keeps everything on the current stream.
_WG_STREAM = os.environ.get("EBSDVAE_WGRAD_STREAM", "1") != "0"
# Inside a hipGraph capture the side stream forks from and joins back into the capturing
# stream (event edges in the graph).  EBSDVAE_GRAPH_SIDE=0 captures on one stream instead.
_GRAPH_SIDE = os.environ.get("EBSDVAE_GRAPH_SIDE", "1") != "0"
# EBSDVAE_LIGHT_EVENTS=0: fork / join through torch's Stream.wait_stream (system-scope fence)
_LIGHT_EVENTS = os.environ.get("EBSDVAE_LIGHT_EVENTS", "1") != "0"
# EBSDVAE_KFORK=0: every fork records an event on the main stream (A/B).  Otherwise the apply
# launch that produces a weight gradient's gy signals the event itself (fork_arm() below), so
# no record packet sits between the apply and the input-gradient conv.
_KFORK = os.environ.get("EBSDVAE_KFORK", "1") != "0"
# EBSDVAE_CU_SPLIT=k (experiment): the side stream runs on k compute units
# (CU-mask bits [N - k, N), N / 8 of them on every XCD) and cu_split_main() gives the other N - k
# to the stream the caller runs the step on, whose persistent conv kernels then launch N - k blocks.
_CU_SPLIT = int(os.environ.get("EBSDVAE_CU_SPLIT", "0"))


class _Lane:
    keep = None    # buffers the side stream uses, dropped at the join (None: idle)
    inside = 0     # > 0 inside run() blocks that made the side stream current

    def __init__(self, stream):
        self.stream = stream


_LANES = {}        # device index -> _Lane
_NO_LANE = _Lane(None)   # a device whose side stream does not exist yet: idle
_SERIAL = 0        # > 0 inside serial_streams()
_JOIN_LATER = 0    # > 0 inside deferred_side_join()


def _dev_key(device):
    return device.index if device.index is not None else torch.cuda.current_device()


@contextlib.contextmanager
def serial_streams():
    """Keep everything on the current stream, e.g. while per-launch durations are measured
    (bench.py's probed steps): overlapped launches are timed with each other's work inside."""
    global _SERIAL
    _SERIAL += 1
    try:
        yield
    finally:
        _SERIAL -= 1


@functools.lru_cache(maxsize=None)
def _cu_stream(key, main: bool):
    ncu = torch.cuda.get_device_properties(key).multi_processor_count
    first, count = (0, ncu - _CU_SPLIT) if main else (ncu - _CU_SPLIT, _CU_SPLIT)
    device = torch.device("cuda", key)
    out = ctypes.c_void_p()
    with torch.cuda.device(device):
        N.call("ebsdvae_stream_create_cus", first, count, ctypes.byref(out))
    return torch.cuda.ExternalStream(out.value, device=device)


def cu_split_main(device):
    """The CU-partitioned main stream of `device` under EBSDVAE_CU_SPLIT (None otherwise)."""
    return _cu_stream(_dev_key(device), True) if _CU_SPLIT > 0 else None


def _lane(device, create=True):
    key = _dev_key(device)
    if key not in _LANES and create:
        side = _cu_stream(key, False) if _CU_SPLIT > 0 else torch.cuda.Stream(device=device)
        _LANES[key] = _Lane(side)
    return _LANES.get(key, _NO_LANE)


def side_stream(device):
    """The side stream of `device` (created on first use; under EBSDVAE_CU_SPLIT, CU-masked)."""
    return _lane(device).stream


def side_streams_enabled() -> bool:
    """Work may go to the side stream now (not disabled, not inside serial_streams(), and not
    a capture that keeps everything on one stream)."""
    return bool(_WG_STREAM and not _SERIAL
                and (_GRAPH_SIDE or not torch.cuda.is_current_stream_capturing()))


def stream_wait(waiter, signaler):
    """`waiter` (a torch Stream) waits for the work enqueued on `signaler` so far."""
    if _LIGHT_EVENTS:
        N.call("ebsdvae_stream_wait", waiter.cuda_stream, signaler.cuda_stream)
    else:
        waiter.wait_stream(signaler)


def fork_arm(device) -> bool:
    """Arm a kernel-attached fork for the next InstanceNorm-backward apply on the current
    stream.  Returns the token for the weight gradient that takes that apply's gy (conv_wgrad's
    fork=); False: nothing armed, the side stream will not take it.  The library keeps the armed
    state per host thread: a later arm replaces it, only a run() holding the token waits on it."""
    if _KFORK and _LIGHT_EVENTS and side_streams_enabled() \
            and not torch.cuda.is_current_stream_capturing():
        N.call("ebsdvae_fork_arm", N.stream())
        return True
    return False


@contextlib.contextmanager
def run(device, *inputs, fork=False, when=True, resume=False):
    """Run the block on `device`'s side stream, forked from the current stream, `inputs` (None
    entries skipped) held until the join.  Yields keep(*tensors), which holds what the block
    allocates too and returns True.  Where the side stream may not take work -- `when` (the
    site's own condition) or side_streams_enabled() is false -- the block runs on the caller's
    stream, nothing is held and keep returns False.
    fork: fork_arm()'s token -- wait for the armed apply launch, not an event recorded now.
    resume: no fork, the block reads only what the side stream wrote; needs a pending lane."""
    lane = _lane(device) if when and side_streams_enabled() else None
    if resume and (lane is None or lane.keep is None):
        raise RuntimeError("side.run(resume=True): the side stream has no work to resume behind")
    if lane is None:
        yield lambda *tensors: False
        return
    if not resume:
        cur = torch.cuda.current_stream(device)
        if fork:
            N.call("ebsdvae_fork_wait", lane.stream.cuda_stream, cur.cuda_stream)
        else:
            stream_wait(lane.stream, cur)
        if lane.keep is None:
            lane.keep = []
    held = lane.keep
    held.extend(t for t in inputs if t is not None)
    lane.inside += 1
    try:
        with torch.cuda.stream(lane.stream):
            yield lambda *tensors: held.extend(tensors) is None
    finally:
        lane.inside -= 1


def inside_run(device) -> bool:
    """A run() block has made `device`'s side stream current (on any thread)."""
    return _lane(device, create=False).inside > 0


def pending(device) -> bool:
    """The side stream took work since the last join."""
    return _lane(device, create=False).keep is not None


def join(device):
    """The current stream waits for the side stream's work so far; the buffers it used are
    released (any later use of them is ordered behind this wait).  Nothing to do when idle."""
    lane = _lane(device, create=False)
    if lane.keep is not None:
        stream_wait(torch.cuda.current_stream(device), lane.stream)
        lane.keep = lane.keep.clear()   # emptied (a keep() still around holds nothing), then None


def join_deferred() -> bool:
    """Inside deferred_side_join(): the block's exit joins, the sites inside do not."""
    return _JOIN_LATER > 0


@contextlib.contextmanager
def deferred_side_join(device):
    """Batched reductions inside the block leave their results on the side stream; the
    current stream joins it once, when the block exits."""
    global _JOIN_LATER
    _JOIN_LATER += 1
    try:
        yield
    finally:
        _JOIN_LATER -= 1
        join(device)
