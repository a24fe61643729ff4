"""The argument handling shared by the evaluation modules (multimodal_supernovae_amd/_device_args.py): the row stride rule,
the accumulator and scratch rules, every refusal with the type and text its callers have always raised, and the life of the
integer accumulators of a validation epoch.  No kernel is launched; what needs a tensor on the GPU is marked gpu."""
import pytest
import torch

from multimodal_supernovae_amd import _device_args as A
from multimodal_supernovae_amd._lib import MsnHipError

GPU_NEEDED = "needs an MI355X"       # _lib.require_gpu on a machine without one


def _raises(exc, text, call):
    with pytest.raises(exc) as e:
        call()
    assert str(e.value) == text


def test_ld_is_the_row_stride_except_that_a_single_row_is_at_least_its_width():
    assert A.ld(torch.zeros(4, 6)) == 6
    assert A.ld(torch.zeros(4, 10)[:, :6]) == 10                             # a row-strided view keeps its stride
    assert A.ld(torch.zeros(1, 7)) == 7
    assert A.ld(torch.zeros(1, 7).as_strided((1, 7), (3, 1))) == 7          # (1, D): the row stride is arbitrary, also odd and below D
    assert A.ld(torch.zeros(1, 7).as_strided((1, 5), (9, 1))) == 9
    assert A.ld(torch.zeros(5, 1)) == 1 and A.ld(torch.zeros(1, 1)) == 1    # C = 1
    assert A.ld(torch.zeros(5, 3)[:, :1]) == 3


def test_accumulator_takes_none_or_exactly_the_tensor_it_describes():
    dev = torch.device("cpu")
    z = A.accumulator(None, (2, 3), dev, "f")
    assert z.shape == (2, 3) and z.dtype == torch.int64 and not z.any()
    mine = torch.ones((2, 3), dtype=torch.int64)
    assert A.accumulator(mine, (2, 3), dev, "f") is mine
    text = "f: the accumulator must be a contiguous int64 (2, 3) tensor on cpu"
    for bad in (torch.ones((3, 2), dtype=torch.int64), torch.ones((2, 3), dtype=torch.int32),
                torch.ones((3, 2), dtype=torch.int64).t(), torch.ones((2, 3), dtype=torch.int64, device="meta")):
        _raises(ValueError, text, lambda: A.accumulator(bad, (2, 3), dev, "f"))


def test_workspace_is_bytes_and_never_empty():
    for nbytes, want in ((0, 8), (5, 8), (8, 8), (4097, 4097)):
        ws = A.workspace(nbytes, "cpu")
        assert ws.dtype == torch.uint8 and ws.numel() == want


def test_rows_are_refused_with_the_callers_types_and_texts():
    S = torch.zeros(4, 3)
    _raises(MsnHipError, "f: scores must live on the GPU (got cpu); there is no CPU path", lambda: A.rows_on_gpu(S, "f", "scores", 8))
    # scores: what the argument is comes before where it lives
    _raises(ValueError, "f: scores must be a float32 (N, C) tensor (got torch.float64 (4, 3))", lambda: A.rows_on_gpu(S.double(), "f", "scores", 8))
    _raises(ValueError, "f: scores must be a float32 (N, C) tensor (got torch.float32 (3,))", lambda: A.rows_on_gpu(S[0], "f", "scores"))
    _raises(ValueError, "f: scores must be a float32 (N, C) tensor (got float32 (4, 3))", lambda: A.rows_on_gpu(S.numpy(), "f", "scores"))
    # embeddings: where comes first, whatever the dtype
    for X in (S, S.double(), S.numpy()):
        with pytest.raises(MsnHipError, match="f: embeddings must live on the GPU" if torch.cuda.is_available() else GPU_NEEDED):
            A.rows_on_gpu(X, "f", "embeddings")


def test_targets_are_refused_with_the_callers_types_and_texts():
    S, y = torch.zeros(4, 3), torch.zeros(4, dtype=torch.int64)
    assert torch.equal(A.targets_next_to(S, y, "f"), y)
    assert A.targets_next_to(S, torch.zeros(8, dtype=torch.int64)[::2], "f").is_contiguous()
    _raises(ValueError, "f: targets must be an int64 tensor of shape (4,) (got torch.int32 (4,))", lambda: A.targets_next_to(S, y.int(), "f"))
    _raises(ValueError, "f: targets must be an int64 tensor of shape (4,) (got torch.int64 (0,))", lambda: A.targets_next_to(S, y[:0], "f"))
    _raises(ValueError, "f: targets must be an int64 tensor of shape (4,) (got list ())", lambda: A.targets_next_to(S, [0, 1, 2, 3], "f"))
    _raises(MsnHipError, "f: targets must live on the GPU next to the scores (got meta); there is no CPU path",
            lambda: A.targets_next_to(S, y.to("meta"), "f"))
    _raises(MsnHipError, "f: scores must live on the GPU (got cpu); there is no CPU path", lambda: A.scores_and_targets(S, y, "f"))


class _Counts(A.EpochCounts):
    _counts = ("first", "second")

    def __init__(self):
        self.first = self.second = None
        self.asked = []

    def _buffers(self, device):
        self.asked.append(device)


def test_reset_zeroes_what_exists_and_leaves_the_rest_unallocated():
    m = _Counts()
    m.reset()
    assert m.first is None and m.second is None
    m.second = torch.arange(6).reshape(2, 3)
    kept = m.second
    m.reset()
    assert m.first is None and m.second is kept and not kept.any()
    assert m.all_reduce() is None and m._all_reduce_counts(None, None) is None and m.asked == []     # a world of one: nothing to do


@pytest.mark.gpu
def test_rows_on_the_gpu_keep_a_usable_stride_and_refuse_no_rows():
    X = torch.zeros(6, 8, device="cuda")
    for noun in ("scores", "embeddings"):
        assert A.rows_on_gpu(X, "f", noun).data_ptr() == X.data_ptr()
        view = A.rows_on_gpu(X[:, :5], "f", noun)
        assert view.data_ptr() == X.data_ptr() and A.ld(view) == 8           # a row stride >= C is kept
        assert A.rows_on_gpu(X.t(), "f", noun).is_contiguous()               # a column stride is not
        assert A.rows_on_gpu(X[:, ::2], "f", noun).is_contiguous()
        _raises(ValueError, "f: no rows", lambda: A.rows_on_gpu(X[:0], "f", noun))
    _raises(MsnHipError, "f: 1 to 4 classes (got 8)", lambda: A.rows_on_gpu(X, "f", "scores", 4))
    _raises(ValueError, "f: embeddings must be float32 (N, D) (got torch.float64 (6, 8))", lambda: A.rows_on_gpu(X.double(), "f", "embeddings"))
    _raises(MsnHipError, "f: embeddings must live on the GPU (got cpu); there is no CPU path", lambda: A.rows_on_gpu(X.double().cpu(), "f", "embeddings"))
    _raises(MsnHipError, "f: targets must live on the GPU next to the scores (got cpu); there is no CPU path",
            lambda: A.scores_and_targets(X, torch.zeros(6, dtype=torch.int64), "f"))
