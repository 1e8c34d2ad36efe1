"""The host layer's bookkeeping that needs no device: ``engine.Stamp`` / ``engine.holds`` (is a stored result still what
it was computed from?) and the reading of ``NFS_GRAPH``."""
import pytest
import torch


def _advance_to(t, version):
    while t._version < version:
        torch.autograd.graph.increment_version(t)
    assert t._version == version


def test_stamp_holds_for_the_same_unmodified_tensors_only():
    from neural_flow_style_amd.engine import Stamp, holds
    a, b = torch.zeros(5), torch.ones(3, 2)
    s = Stamp(a, b)
    assert holds(s, a, b) and holds(s, a, b)                   # (asking changes nothing)
    assert holds(Stamp(a), a)
    # the order is part of it
    assert not holds(s, b, a)
    # a shorter or a longer tensor list
    assert not holds(s, a) and not holds(s, a, b, a) and not holds(s)
    # no stamp, an empty stamp
    assert not holds(None, a, b) and not holds(None)
    assert not holds(Stamp(), a) and not holds(Stamp())
    # a missing tensor where one was stamped (TFAdamState before its first step)
    assert not holds(s, None, None)


@pytest.mark.parametrize("write", ["inplace", "detach_view", "increment_version"])
@pytest.mark.parametrize("which", [0, 1])
def test_stamp_is_stale_after_a_write_to_any_of_its_tensors(write, which):
    from neural_flow_style_amd.engine import Stamp, holds
    ts = [torch.zeros(4), torch.ones(2, 3)]
    s = Stamp(*ts)
    if write == "inplace":
        ts[which].mul_(1.0)                                    # (a no-op in value: the counter moves all the same)
    elif write == "detach_view":
        ts[which].detach().add_(1.0)                           # (views share the version counter)
    else:
        torch.autograd.graph.increment_version(ts[which])
    assert not holds(s, *ts)
    assert holds(Stamp(*ts), *ts)                              # ... and a stamp taken now holds again


def test_stamp_is_stale_for_another_tensor_whose_version_collides():
    """versions alone do not identify a tensor: a re-bound tensor whose counter happens to equal the recorded one is
    another tensor (the collision a key of version numbers only cannot see)"""
    from neural_flow_style_amd.engine import Stamp, holds
    m, v = torch.zeros(6), torch.zeros(6)
    m.add_(1.0); m.add_(1.0); v.add_(1.0)
    s = Stamp(m, v)
    m2 = m + 1e-3                                              # a new tensor: version 0
    _advance_to(m2, m._version)
    assert (m2._version, v._version) == (m._version, v._version)
    assert not holds(s, m2, v)
    assert holds(s, m, v)                                      # the stamped pair itself is untouched by all that
    clone = m.clone()
    _advance_to(clone, m._version)
    assert torch.equal(clone, m) and not holds(s, clone, v)    # (equal values, equal versions: still another tensor)


def test_stamp_allocates_no_tensor_and_keeps_no_dict():
    from neural_flow_style_amd.engine import Stamp
    s = Stamp(torch.zeros(2))
    assert not hasattr(s, "__dict__")
    with pytest.raises(AttributeError):
        s.other = 1


@pytest.mark.parametrize("value,expected", [(None, None), ("1", True), ("0", False), ("", False)])
def test_graph_from_env_reads_nfs_graph(monkeypatch, value, expected):
    from neural_flow_style_amd.engine import graph_from_env
    if value is None:
        monkeypatch.delenv("NFS_GRAPH", raising=False)
    else:
        monkeypatch.setenv("NFS_GRAPH", value)
    assert graph_from_env() is expected


@pytest.mark.parametrize("value,force", [(None, None), ("1", True)])
def test_graphed_loss_from_env_is_the_one_constructor_path(monkeypatch, value, force):
    from neural_flow_style_amd.engine import GraphedLoss
    loss = object()
    if value is None:
        monkeypatch.delenv("NFS_GRAPH", raising=False)
    else:
        monkeypatch.setenv("NFS_GRAPH", value)
    g = GraphedLoss.from_env(loss)
    assert isinstance(g, GraphedLoss) and g.loss is loss and g.force is force and g._graph is None
    assert g.mode == (None if force is None else "graph")
    monkeypatch.setenv("NFS_GRAPH", "0")
    assert GraphedLoss.from_env(loss) is False                 # (off: the stylers call the loss directly)


def test_adam_state_advances_its_beta_powers_without_an_update_as_a_step_does():
    import numpy as np
    from neural_flow_style_amd.engine import TFAdamState
    idle, stepping = TFAdamState(), TFAdamState()
    x = torch.zeros(3)
    for _ in range(3):
        idle.advance()
        stepping._begin_step(x, 0.1)
    assert idle.b1p == stepping.b1p and idle.b2p == stepping.b2p
    assert idle.b1p.dtype == np.float32 and idle.m is None and idle.ever_mask() is None
