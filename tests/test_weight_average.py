"""The averaging launch alone (csrc/weight_average.hip, include/aqgnn.h "weight averaging"): bit for bit
train_network.weight_average_reference on tensor sizes around the 16-byte word, the wave, the workgroup and the chunk, 1, 2 and 17
tensors per launch, every offset of both bases inside 16 bytes, inside NaN margins that must stay NaN -- and every refusal of the
library, the average untouched."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

pytestmark = pytest.mark.gpu

C = 4096                                   # AQG_WEIGHT_AVERAGE_CHUNK
SIZES = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, C - 1, C, C + 1, 2 * C + 1)
MIXED = SIZES + (1000, 2, C + 7)           # 17 tensors of mixed sizes
DECAYS = (0.0, 0.5, 0.999, 1.0 - 2.0 ** -24)
MARGIN = 8                                 # floats of NaN on either side of every average tensor (a multiple of 4)


@pytest.fixture(scope="module")
def dev():
    from alphaquoridorgnn_amd import _lib
    _lib.load()
    return _lib.require_gpu()


class _Case:
    """Average tensors of `sizes` inside one NaN-filled device buffer, tensor i at `aoff[i]` floats behind a 16-byte boundary, and
    their sources inside a buffer of finite values at `soff[i]` floats behind one; the launch's struct over them."""

    def __init__(self, dev, sizes, aoff, soff, decay, seed=0, every=1):
        from alphaquoridorgnn_amd import _lib
        from alphaquoridorgnn_amd.train_network import weight_average_table
        rng = np.random.RandomState(seed)
        slots = [(n + 3) // 4 * 4 + 4 + 2 * MARGIN for n in sizes]             # 16-byte multiples: every slot starts on the grid
        starts = np.concatenate([[0], np.cumsum(slots)]).astype(int)
        self.arange = [(int(starts[i]) + MARGIN + aoff[i], n) for i, n in enumerate(sizes)]
        self.srange = [(int(starts[i]) + MARGIN + soff[i], n) for i, n in enumerate(sizes)]
        self.avg_host = np.full(int(starts[-1]), np.nan, np.float32)
        for lo, n in self.arange:
            self.avg_host[lo:lo + n] = rng.randn(n).astype(np.float32)
        self.src_host = rng.randn(int(starts[-1])).astype(np.float32)
        self.avg, self.src = torch.from_numpy(self.avg_host).to(dev), torch.from_numpy(self.src_host).to(dev)
        assert self.avg.data_ptr() % 16 == 0 and self.src.data_ptr() % 16 == 0
        self.averages = [self.avg[lo:lo + n] for lo, n in self.arange]
        self.sources = [self.src[lo:lo + n] for lo, n in self.srange]
        self.host_table, self.table, self.chunks = weight_average_table(self.averages, self.sources)
        self.lib, self.dev, self.decay = _lib.load(), dev, decay
        self.a = _lib.WeightAverageStruct()
        self.a.table = self.table.data_ptr()
        self.a.host_table = ctypes.cast(self.host_table, ctypes.POINTER(ctypes.c_int64))
        self.a.num_tensors, self.a.every, self.a.total_chunks, self.a.decay = len(sizes), every, self.chunks, decay

    def launch(self):
        from alphaquoridorgnn_amd import _lib
        return self.lib.aqg_weight_average_update(ctypes.byref(self.a), _lib.stream_ptr(self.dev))

    def expected(self):
        from alphaquoridorgnn_amd.train_network import weight_average_reference
        want = self.avg_host.copy()
        for (lo, n), (slo, _) in zip(self.arange, self.srange):
            want[lo:lo + n] = weight_average_reference(self.avg_host[lo:lo + n], self.src_host[slo:slo + n], self.decay)
        return want

    def check(self, what):
        """The whole average buffer -- every updated element and every NaN of the margins -- and the whole source buffer, bit for bit."""
        assert self.launch() == 0, self.lib.aqg_last_error()
        got = self.avg.cpu().numpy()
        assert np.array_equal(got.view(np.uint32), self.expected().view(np.uint32)), what
        assert np.array_equal(self.src.cpu().numpy().view(np.uint32), self.src_host.view(np.uint32)), what

    def untouched(self):
        torch.cuda.synchronize()
        return np.array_equal(self.avg.cpu().numpy().view(np.uint32), self.avg_host.view(np.uint32))


@pytest.mark.parametrize("decay", DECAYS)
def test_one_tensor_every_size(dev, decay):
    """T = 1, each size alone, both bases on the grid (the trainers' case) and the average one float, the source three floats off it."""
    for n in SIZES:
        for ao, so in ((0, 0), (1, 3)):
            _Case(dev, (n,), (ao,), (so,), decay, seed=n).check((decay, n, ao, so))


def test_two_tensors_every_pair_of_offsets(dev):
    """T = 2: average and source bases offset by 0 .. 3 floats from a 16-byte boundary, independently -- the 16-byte path where the two
    sit alike, float by float where they do not; one tensor below a word and one above a chunk."""
    for ao in range(4):
        for so in range(4):
            _Case(dev, (5, C + 1), (ao, (ao + 1) % 4), (so, (so + 3) % 4), 0.999, seed=4 * ao + so).check((ao, so))
            _Case(dev, (C, 3), (ao, ao), (so, so), 0.5, seed=16 + 4 * ao + so).check((ao, so))


@pytest.mark.parametrize("decay", DECAYS)
def test_seventeen_mixed_tensors_in_one_launch(dev, decay):
    """T = 17, every size of the list in ONE launch (26 chunks), all sixteen pairs of offsets, then each tensor with its own pair."""
    assert len(MIXED) == 17
    for ao in range(4):
        for so in range(4):
            _Case(dev, MIXED, (ao,) * 17, (so,) * 17, decay, seed=ao + 4 * so).check((decay, ao, so))
    own = _Case(dev, MIXED, tuple(i % 4 for i in range(17)), tuple((3 * i + 1) % 4 for i in range(17)), decay, seed=99)
    assert own.chunks == sum((n + i % 4 + C - 1) // C for i, n in enumerate(MIXED))
    own.check((decay, "own offsets"))


def test_repeated_updates_follow_the_reference(dev):
    """Five updates in a row with the source changing in between, as a trainer's steps change it."""
    from alphaquoridorgnn_amd.train_network import weight_average_reference
    case = _Case(dev, (257, C + 1, 64), (0, 0, 0), (0, 0, 0), 0.9, seed=7)
    want = [case.avg_host[lo:lo + n].copy() for lo, n in case.arange]
    for k in range(5):
        assert case.launch() == 0
        want = [weight_average_reference(w, s.cpu().numpy(), 0.9) for w, s in zip(want, case.sources)]
        case.src.mul_(0.5).add_(float(k))
    for e, w in zip(case.averages, want):
        assert np.array_equal(e.cpu().numpy().view(np.uint32), w.view(np.uint32))


def test_library_refusals_leave_the_average_untouched(dev):
    from alphaquoridorgnn_amd import _lib
    from alphaquoridorgnn_amd.train_network import weight_average_table
    lib = _lib.load()

    def refused(case, what):
        assert case.launch() == -1, what
        assert b"aqg_weight_average_update" in lib.aqg_last_error(), what
        assert case.untouched(), what

    def fresh():
        return _Case(dev, (5, C + 1, 64), (0, 1, 2), (0, 1, 3), 0.9, seed=1)

    assert lib.aqg_weight_average_update(None, _lib.stream_ptr(dev)) == -1                   # a NULL struct
    for field, value in (("table", None), ("host_table", ctypes.POINTER(ctypes.c_int64)()), ("num_tensors", 0), ("num_tensors", -1),
                         ("num_tensors", _lib.WEIGHT_AVERAGE_MAX_TENSORS + 1), ("decay", -0.1), ("decay", 1.0), ("decay", 1.5),
                         ("decay", float("nan")), ("decay", float("inf")), ("every", 0), ("every", -2), ("total_chunks", 3),
                         ("total_chunks", 5)):                                   # (the case has 1 + 2 + 1 = 4 chunks)
        case = fresh()
        setattr(case.a, field, value)
        refused(case, (field, value))
    T = 3
    for word, value, what in ((2 * T + 1, 0, "a tensor of 0 elements"), (2 * T + 1, -5, "a negative element count"),
                              (0, 0, "a NULL average"), (T + 2, 0, "a NULL source"), (1, None, "an average off the 4-byte grid"),
                              (3 * T, 1, "a prefix that does not start at 0"), (3 * T + 2, 7, "a prefix that is not the tensors'"),
                              (2 * T + 1, 3 * C, "an element count the prefix does not cover")):
        case = fresh()
        case.host_table[word] = case.host_table[word] + 2 if value is None else value
        refused(case, what)
    # overlaps: an average inside a source, a source that ends inside an average, an average inside another average
    case = fresh()
    for averages, sources, what in (
            ([case.src[40:45]], [case.src[43:48]], "an average that overlaps its own source"),
            ([case.avg[8:13], case.avg[40:104]], [case.src[8:13], case.avg[0:64]], "a source that ends inside another tensor's average"),
            ([case.avg[8:72], case.avg[71:76]], [case.src[8:72], case.src[100:105]], "two averages that share a float"),
            ([case.avg[8:13]], [case.avg[8:13]], "a tensor averaged into itself")):
        other = fresh()
        other.avg, other.avg_host = case.avg, case.avg_host
        other.host_table, other.table, other.chunks = weight_average_table(averages, sources)
        other.a.table = other.table.data_ptr()
        other.a.host_table = ctypes.cast(other.host_table, ctypes.POINTER(ctypes.c_int64))
        other.a.num_tensors, other.a.total_chunks = len(averages), other.chunks
        src_before = case.src.clone()
        refused(other, what)
        assert torch.equal(case.src, src_before), what
    # two sources may be one tensor (read only): not refused
    shared = _Case(dev, (5, 5), (0, 0), (0, 0), 0.5, seed=2)
    shared.sources = [shared.sources[0], shared.sources[0]]
    shared.srange = [shared.srange[0], shared.srange[0]]
    shared.host_table, shared.table, shared.chunks = weight_average_table(shared.averages, shared.sources)
    shared.a.table = shared.table.data_ptr()
    shared.a.host_table = ctypes.cast(shared.host_table, ctypes.POINTER(ctypes.c_int64))
    shared.check("two averages of one source")
