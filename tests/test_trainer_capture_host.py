"""Host logic around the captured training step (no GPU): the static copies of a batch, the scaffold that maps a refused
collective to ``CollectiveCaptureRefused``, and the protocol by which the ranks settle ``collective_mode``."""
import dataclasses
from unittest import mock

import pytest
import torch
import torch.distributed as dist

from equihgnn_amd.batch import synth_batch, synth_graph_batch
from equihgnn_amd.prefetch import copy_into_static, static_copy_of
from equihgnn_amd.trainer import CollectiveCaptureRefused, GraphedTrainStep, capture_graph


@dataclasses.dataclass
class _Plain:
    """A batch type without ``packed()``: the field-by-field routes."""
    x: torch.Tensor
    y: torch.Tensor
    name: str = "plain"


def _tensor_fields(b):
    return {f: getattr(b, f) for f in b.__dataclass_fields__ if torch.is_tensor(getattr(b, f))}


def _assert_same_values(a, b, distinct):
    fa, fb = _tensor_fields(a), _tensor_fields(b)
    assert fa.keys() == fb.keys() and fa
    for f in fa:
        assert torch.equal(fa[f], fb[f]) and fa[f].dtype == fb[f].dtype, f
        if distinct and fa[f].numel():
            assert fa[f].untyped_storage().data_ptr() != fb[f].untyped_storage().data_ptr(), f


BATCHES = {"hyper": lambda seed: synth_batch(2, seed), "hyper_packed": lambda seed: synth_batch(2, seed).packed(),
           "graph_2d": lambda seed: synth_graph_batch(2, seed), "graph_2d_packed": lambda seed: synth_graph_batch(2, seed).packed(),
           "plain": lambda seed: _Plain(torch.arange(6.0).reshape(2, 3) + seed, torch.tensor([1.0, float(seed)]))}


@pytest.mark.parametrize("kind", list(BATCHES))
def test_static_copy_of_gives_equal_tensors_in_storage_of_its_own(kind):
    data = BATCHES[kind](41)
    data.num_real_graphs = 2
    static = static_copy_of(data)
    assert type(static) is type(data) and static.num_real_graphs == 2
    _assert_same_values(static, data, distinct=True)
    assert hasattr(static, "_flat") == (kind != "plain")        # packed where the batch type can be
    if kind == "plain":
        assert static.name == "plain"
    del data.num_real_graphs
    assert static_copy_of(data).num_real_graphs is None


@pytest.mark.parametrize("kind", list(BATCHES))
def test_copy_into_static_takes_one_copy_when_the_layouts_match_and_the_fields_otherwise(kind):
    static, data = static_copy_of(BATCHES[kind](41)), BATCHES[kind](41)
    for t in _tensor_fields(static).values():     # (same extents, other contents: the copy has something to do)
        t.zero_()
    one_copy = kind.endswith("_packed")
    assert (getattr(data, "_layout", None) is not None and data._layout == getattr(static, "_layout", None)) == one_copy
    real, calls = torch.Tensor.copy_, []

    def counted(self, src, non_blocking=False):
        calls.append(self)
        return real(self, src, non_blocking=non_blocking)
    with mock.patch.object(torch.Tensor, "copy_", counted):
        copy_into_static(static, data)
    if one_copy:
        assert len(calls) == 1 and calls[0] is static._flat
    else:
        assert len(calls) == len(_tensor_fields(data))
    _assert_same_values(static, data, distinct=True)


# ---- the capture scaffold --------------------------------------------------------------------------------------------------
class _Context:
    """Stands in for ``torch.cuda.graph``: ending a capture that a refused collective invalidated raises again."""

    def __init__(self, graph, capture_error_mode):
        assert capture_error_mode == "thread_local"
        self.graph = graph

    def __enter__(self):
        self.graph["open"] = True

    def __exit__(self, kind, exc, tb):
        self.graph["open"] = False
        if exc is None and self.graph.get("invalidated"):
            raise RuntimeError("capture_end: the capture was invalidated")
        return False


def _raiser(exc):
    def call():
        raise exc
    return call


def test_capture_graph_returns_the_graph_and_what_the_body_returned():
    g, seen = {}, []

    def body(collective):
        assert g["open"] and collective(lambda: seen.append("all_reduce"))
        return "loss"
    assert capture_graph(body, g, _Context) == (g, "loss") and seen == ["all_reduce"] and not g["open"]


@pytest.mark.parametrize("ending_raises", [True, False])
def test_capture_graph_turns_a_refused_collective_and_nothing_else_into_the_refusal(ending_raises):
    boom, g, after = RuntimeError("collective not capturable"), {}, []

    def body(collective):
        if not collective(_raiser(boom)):
            g["invalidated"] = ending_raises
            return None
        after.append("update")
    with pytest.raises(CollectiveCaptureRefused, match="RuntimeError: collective not capturable") as info:
        capture_graph(body, g, _Context)
    assert info.value.__cause__ is boom and not after and not g["open"]
    # an error anywhere else in the body is itself, and so is a collective's error that is no RuntimeError
    launch = RuntimeError("kernel launch failed")
    with pytest.raises(RuntimeError) as info:
        capture_graph(lambda collective: _raiser(launch)(), {}, _Context)
    assert info.value is launch and not isinstance(info.value, CollectiveCaptureRefused)
    with pytest.raises(ValueError):
        capture_graph(lambda collective: collective(_raiser(ValueError("bad argument"))), {}, _Context)


# ---- settling the collective mode among the ranks --------------------------------------------------------------------------
def _settler(monkeypatch, agreed, refuse=False, backend="nccl", **kw):
    """A multi-rank trainer (never stepped: no process group, no device) with a stand-in agreement, and capture(in_graph)."""
    monkeypatch.setattr(dist, "get_backend", lambda: backend)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda: None)
    tr = GraphedTrainStep(torch.nn.Linear(2, 1), **kw)
    tr._multi = lambda: True
    log = {"captures": [], "asked": [], "abandoned": 0}

    def agree(mode):
        log["asked"].append(mode)
        return agreed or mode
    tr._agree_on_mode = agree

    def capture(in_graph):
        log["captures"].append(in_graph)
        if in_graph and refuse:
            raise CollectiveCaptureRefused("DistBackendError: not capturable")
        return "in-graph capture" if in_graph else "split capture"

    def abandoned():
        log["abandoned"] += 1
    return tr, log, lambda: tr._settle_mode(capture, abandoned)


def test_settle_mode_keeps_the_in_graph_capture_when_every_rank_has_one(monkeypatch):
    tr, log, settle = _settler(monkeypatch, agreed=None)
    assert settle() == "in-graph capture" and tr.collective_mode == "in_graph" and tr.capture_error is None
    assert log == {"captures": [True], "asked": ["in_graph"], "abandoned": 0}
    assert settle() == "in-graph capture" and log["asked"] == ["in_graph"]         # the ranks agree once


def test_settle_mode_falls_back_to_split_when_the_first_capture_is_refused(monkeypatch):
    tr, log, settle = _settler(monkeypatch, agreed=None, refuse=True)
    assert settle() == "split capture" and tr.collective_mode == "split"
    assert tr.capture_error == "DistBackendError: not capturable"
    assert log == {"captures": [True, False], "asked": ["split"], "abandoned": 1}
    assert settle() == "split capture" and log["captures"] == [True, False, False]  # split binds the later captures


def test_settle_mode_raises_when_a_capture_is_refused_after_the_ranks_agreed_on_in_graph(monkeypatch):
    tr, log, settle = _settler(monkeypatch, agreed=None, refuse=True)
    tr._mode_agreed, tr.collective_mode = True, "in_graph"      # (an earlier bucket's capture settled it)
    with pytest.raises(RuntimeError, match="GraphedTrainStep: the ranks agreed on the in-graph all-reduce at the first capture "
                                           r"and this rank can no longer capture it \(DistBackendError: not capturable\)") as info:
        settle()
    assert isinstance(info.value.__cause__, CollectiveCaptureRefused) and not isinstance(info.value, CollectiveCaptureRefused)
    assert log == {"captures": [True], "asked": [], "abandoned": 0} and tr.collective_mode == "in_graph"


def test_settle_mode_drops_its_graph_to_follow_a_rank_that_could_not_capture(monkeypatch):
    tr, log, settle = _settler(monkeypatch, agreed="split")
    assert settle() == "split capture" and tr.collective_mode == "split"
    assert tr.capture_error == "another rank could not capture the collective"
    assert log == {"captures": [True, False], "asked": ["in_graph"], "abandoned": 1}


@pytest.mark.parametrize("how", ["graph_collective_off", "backend_not_capturable"])
def test_settle_mode_never_attempts_in_graph_where_it_is_ruled_out(monkeypatch, how):
    kw = {"graph_collective": False} if how == "graph_collective_off" else {}
    tr, log, settle = _settler(monkeypatch, agreed=None, backend="nccl" if kw else "gloo", **kw)
    assert settle() == "split capture" and tr.collective_mode == "split" and tr.capture_error is None
    assert log == {"captures": [False], "asked": ["split"], "abandoned": 0}


def test_settle_mode_of_a_single_rank_captures_once_without_asking_anyone(monkeypatch):
    tr, log, settle = _settler(monkeypatch, agreed=None)
    tr._multi = lambda: False
    assert settle() == "split capture" and tr.collective_mode == "none"
    assert log == {"captures": [False], "asked": [], "abandoned": 0}
