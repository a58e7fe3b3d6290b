"""Host-side bookkeeping of the weight-gradient side stream's lane (latice/side.py): what it
holds and until when, and that side.run() is the only way the side stream becomes current
during a trainer step.  Nothing here tries to make a race observable."""
import weakref

import numpy as np
import pytest
import torch

from pinned import fixture
from latice import _native as N
from latice import side as S
from latice.model import VariationalAutoEncoderRawData
from latice.trainer import VAETrainer

pytestmark = pytest.mark.gpu


@pytest.fixture
def lane(cuda, monkeypatch):
    """An idle lane with the side stream switched on, whatever the environment says."""
    monkeypatch.setattr(S, "_WG_STREAM", True)
    S.join(cuda)
    assert not S.pending(cuda)
    yield cuda
    S.join(cuda)
    torch.cuda.synchronize()


def test_lane_holds_inputs_and_kept_buffers_until_the_join(lane):
    side = S.side_stream(lane)
    main = torch.cuda.current_stream(lane)
    a = torch.ones(48, device=lane)
    with S.run(lane, a, None) as keep:
        assert torch.cuda.current_stream(lane) == side and S.inside_run(lane)
        b = torch.zeros(32, device=lane)
        assert keep(b) is True
    assert torch.cuda.current_stream(lane) == main and not S.inside_run(lane)
    refs = [weakref.ref(a), weakref.ref(b)]
    del a, b
    assert S.pending(lane)
    assert all(r() is not None for r in refs)
    S.join(lane)
    assert not S.pending(lane)
    assert all(r() is None for r in refs)


def test_serial_streams_keeps_the_block_on_the_callers_stream(lane):
    main = torch.cuda.current_stream(lane)
    a = torch.ones(48, device=lane)
    with S.serial_streams():
        with S.run(lane, a) as keep:
            assert torch.cuda.current_stream(lane) == main and not S.inside_run(lane)
            b = torch.zeros(32, device=lane)
            assert keep(b) is False
        assert not S.pending(lane)
    refs = [weakref.ref(a), weakref.ref(b)]
    del a, b
    assert all(r() is None for r in refs)
    with S.run(lane, when=False):
        assert torch.cuda.current_stream(lane) == main
    assert not S.pending(lane)


def test_resume_needs_a_pending_lane(lane):
    with pytest.raises(RuntimeError, match="resume"):
        with S.run(lane, resume=True):
            pass
    assert not S.pending(lane)
    with S.run(lane):
        pass
    with S.run(lane, resume=True):   # behind the work above: no fork, still pending
        assert torch.cuda.current_stream(lane) == S.side_stream(lane)
    assert S.pending(lane)


def test_side_stream_is_current_only_inside_run(lane, monkeypatch):
    """One trainer step (no collectives): every library call issued while the side stream is
    the current stream comes from inside a side.run() block."""
    f, sd = fixture("vae128_b4")
    m = VariationalAutoEncoderRawData(32, int(f["meta"][2]), int(f["meta"][1]))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    tr = VAETrainer(m.to(lane), kl_lambda=float(f["kl_lambda"]))
    assert not tr.reducer.active
    x = torch.from_numpy(np.ascontiguousarray(f["x"])).to(lane)
    eps = torch.from_numpy(np.ascontiguousarray(f["eps"])).to(lane)
    side = S.side_stream(lane)
    real = N.call
    on_side, on_main, outside = [], [], []

    def call(name, *args):
        if torch.cuda.current_stream(lane) == side:
            on_side.append(name)
            if not S.inside_run(lane):
                outside.append(name)
        else:
            on_main.append(name)
        return real(name, *args)

    monkeypatch.setattr(N, "call", call)
    tr.forward_backward(x, eps)
    torch.cuda.synchronize()
    assert not outside, f"side stream current outside side.run(): {outside}"
    # the step did use both streams, and it left the lane joined
    assert any(n.startswith("ebsdvae_conv3x3_wgrad") for n in on_side)
    assert "ebsdvae_heads_wgrad" in on_side and on_main
    assert not S.pending(lane)
