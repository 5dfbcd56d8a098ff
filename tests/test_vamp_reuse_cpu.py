"""CPU: when `VAMP` tells the library to reuse the workspace's packed operators
(vamp._OperatorReuse, VAMP._run_reusing), with the library call stubbed.

The flag is 1 only when the caller's U, s, Vh are the same tensor objects at the same versions,
the dims / k / iterations / engine / gemm key and the workspace tensor are unchanged, and the
previous forward on that workspace returned; every clear point leaves the next forward building.
"""
import types

import pytest
import torch


def _cfg(B=32):
    from config import Config
    return Config(64, 4, 128, 1, 1, batch=B, generator_mode='sparc', iterations=20, alphabet='QPSK',
                  channel_profile='uniform', channel_truncation='tail', device='cpu')


class _Stub:
    """A VAMP on the CPU whose library call is `call(reuse)`: records the flags it was handed."""

    def __init__(self, cfg=None):
        from vamp import VAMP
        self.cfg = cfg or _cfg()
        self.det = VAMP(self.cfg)
        self.ws = torch.empty(256, dtype=torch.uint8)
        self.flags = []
        self.rc = 0

    def tracker(self, k=64):
        return types.SimpleNamespace(dims=self.det.config.dims(), k=k, y=torch.zeros(1),
                                     buf=types.SimpleNamespace(ws=self.ws))

    def forward(self, U, s, Vh, k=64):
        def call(reuse):
            self.flags.append(reuse)
            return self.rc
        return self.det._run_reusing(self.tracker(k), U, s, Vh, call, 'stub')


def _chan():
    return torch.randn(128, 64, dtype=torch.complex64), torch.rand(64), torch.randn(64, 64, dtype=torch.complex64)


def test_same_objects_reuse_after_a_building_forward():
    st = _Stub()
    U, s, Vh = _chan()
    assert [st.forward(U, s, Vh) for _ in range(3)] == [0, 1, 1]
    assert st.flags == [0, 1, 1]


@pytest.mark.parametrize('which', [0, 1, 2])
def test_version_bump_rebuilds_then_reuse_resumes(which):
    st = _Stub()
    ch = _chan()
    st.forward(*ch)
    assert st.forward(*ch) == 1
    ch[which].mul_(-1)
    assert st.forward(*ch) == 0
    assert st.forward(*ch) == 1


@pytest.mark.parametrize('which', [0, 1, 2])
def test_new_object_with_equal_contents_rebuilds(which):
    st = _Stub()
    ch = list(_chan())
    st.forward(*ch)
    ch[which] = ch[which].clone()
    assert st.forward(*ch) == 0
    assert st.forward(*ch) == 1


def test_key_changes_rebuild():
    import amp_native as nat
    st = _Stub()
    ch = _chan()
    st.forward(*ch)
    st.det.gemm = nat.GEMM_F32
    assert st.forward(*ch) == 0
    assert st.forward(*ch) == 1
    st.det.engine = nat.ENGINE_PERSISTENT
    assert st.forward(*ch) == 0
    assert st.forward(*ch, k=32) == 0          # another k
    st.det.config = _cfg(B=48)                 # other dims
    assert st.forward(*ch, k=32) == 0
    assert st.forward(*ch, k=32) == 1
    st.det.config.N_Layers = 10                # another iteration cap (another workspace carve)
    assert st.forward(*ch, k=32) == 0


def test_another_workspace_rebuilds():
    st = _Stub()
    ch = _chan()
    st.forward(*ch)
    st.ws = torch.empty(256, dtype=torch.uint8)
    assert st.forward(*ch) == 0
    assert st.forward(*ch) == 1


def test_a_forward_that_raises_leaves_no_record():
    import amp_native as nat
    st = _Stub()
    ch = _chan()
    st.forward(*ch)
    st.rc = 1
    with pytest.raises((nat.AmpError, RuntimeError)):
        st.forward(*ch)
    assert st.flags[-1] == 1                   # it was a reuse forward that failed
    st.rc = 0
    assert st.forward(*ch) == 0
    assert st.forward(*ch) == 1


def test_clear_points(monkeypatch):
    """A grid rescue, forward_epochs, forward_trials and ShardedVAMP's forward drop the record."""
    import vamp
    st = _Stub()
    ch = _chan()

    def armed():
        st.det._ops.clear()
        st.forward(*ch)
        assert st.forward(*ch) == 1

    class Stop(Exception):
        pass

    def stop(*a, **k):
        raise Stop

    # each of these drops the record first and then fails on the CPU tensors it was handed (no
    # ROCm device here), before any library call
    y = torch.zeros(1)
    armed()
    with pytest.raises(ValueError):
        st.det._rescue_forward(*ch, y, 1.0, None, None, None)
    assert st.forward(*ch) == 0

    armed()
    with pytest.raises(ValueError):
        st.det.forward_epochs(*ch, [y], 1.0, [None], [None], [None])
    assert st.forward(*ch) == 0

    armed()
    monkeypatch.setattr(st.det, '_trials_check', lambda *a: 1)
    with pytest.raises(ValueError):
        st.det.forward_trials(*ch, [y], 1.0, [None], [None], [None])
    assert st.forward(*ch) == 0

    sh = vamp.ShardedVAMP(st.cfg)
    sh._ops.begin(*ch, 'key', st.ws)
    sh._ops.commit()
    monkeypatch.setattr(sh, 'shard', stop)
    with pytest.raises(Stop):
        sh._forward(*ch, torch.zeros(1), 1.0, None, None, None)
    assert sh._ops.begin(*ch, 'key', st.ws) == 0


def test_strong_references():
    """The record keeps the channel objects alive: a freed channel's address cannot come back as
    a new tensor that passes for the old one."""
    import weakref
    st = _Stub()
    U, s, Vh = _chan()
    refs = [weakref.ref(t) for t in (U, s, Vh)]
    st.forward(U, s, Vh)
    del U, s, Vh
    assert all(r() is not None for r in refs)
    st.det._ops.clear()
    assert all(r() is None for r in refs)
