"""The staged device-to-host copy on the GPU (csrc/mm_hostcopy.hip; its arithmetic and ordering protocol without one:
tests/test_hostcopy_host.py).  Every sample that reaches a caller's host array passes through mm_copy_to_host, so a test that
compares two host results cannot see a copy error.  The reference here is NOT the library's copy: two handles with the same
seed produce the same device data (bit for bit, as the suite shows elsewhere); one writes a torch device tensor that torch's
own .cpu() fetches, the other writes a host buffer through the library, and all bytes must be equal.

  * a table of byte counts around every edge of the protocol -- the direct / staged threshold (4 MiB), one chunk (8 MiB), the
    ring of four (32 MiB), the first slot reuse, last chunks of 4, 12 and 4100 bytes -- with the integer-state MH as producer
    ([C, n, 1] int32) into a caller-owned buffer between two guards of 0x5a;
  * destinations: page-aligned, 4 bytes past a page, pinned (the direct branch);
  * every caller of mm_copy_to_host once above 8 MiB with a ragged tail;
  * three copies in flight together from three Python threads (ctypes releases the GIL for the call);
  * fresh processes narrowed to 1, 2, 6 and up to 16 CPUs (tests/hostcopy_child.py): the plain copy, and 1, 3 and up to 8 copy
    threads."""
import ctypes as C
import hashlib
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "hostcopy_child.py")
MiB = 1 << 20
GUARD = 64
# bytes -> (chains, n_collect) of the integer-state MH sample: chains * n_collect * 4 = bytes, at least 3 chains
# (2^20 - 1 = 1025 * 1023, 2^20 + 1 = 17 * 61681, 2^21 - 1 = 889 * 2359, 2^21 + 1 = 387 * 5419, 2^23 + 1 = 2796203 * 3,
# 10 * 2^20 + 1025 = 699119 * 15, 18 * 2^20 + 3 = 1041 * 18131)
SHAPES = {
    4 * MiB - 4: (1025, 1023),     # the last direct copy
    4 * MiB: (1024, 1024),         # the first staged one: half a chunk
    4 * MiB + 4: (17, 61681),      # few long chains; half a chunk and four bytes
    8 * MiB - 4: (889, 2359),      # one chunk, four bytes short
    8 * MiB: (2048, 1024),         # exactly one chunk
    8 * MiB + 4: (387, 5419),      # a second chunk of four bytes: only copy thread 0 has work in it
    32 * MiB: (4096, 2048),        # exactly the ring: no slot is used twice
    32 * MiB + 4: (2796203, 3),    # the fifth chunk, the first reuse of a slot, four bytes
    40 * MiB + 4100: (699119, 15),  # two slots reused; a last chunk of one page and four bytes
    72 * MiB + 12: (1041, 18131),  # every slot reused, slot 0 three times
}
N_DISCARD = 3


def _name(nbytes):
    """4194300 -> 4MiB-4"""
    whole = (nbytes + MiB // 2) // MiB
    return f"{whole}MiB{nbytes - whole * MiB:+d}" if nbytes % MiB else f"{whole}MiB"


def producer(nbytes):
    """a fresh integer-state MH handle whose run(SHAPES[nbytes][1], N_DISCARD) is `nbytes` of sample; the same data every time"""
    from mini_mcmc_amd import discrete as D

    chains, _ = SHAPES[nbytes]
    assert chains >= 3 and chains * SHAPES[nbytes][1] * 4 == nbytes
    return D.DiscreteMetropolisHastings(D.PoissonReflect(4.0), (np.arange(chains) % 9).astype(np.int32)).seed(1000 + chains)


class Dest:
    """`nbytes` of caller-owned host memory inside a buffer prefilled with 0x5a, at least GUARD bytes of it on either side;
    page_offset: None = 64 bytes into the buffer wherever that is, else the destination's address modulo 4096"""

    def __init__(self, nbytes, page_offset=None, pinned=False):
        total = nbytes + 2 * GUARD + (0 if page_offset is None else 4096)
        if pinned:
            import torch

            self._keep = torch.empty(total, dtype=torch.uint8, pin_memory=True)
            self.buf = self._keep.numpy()
            self.buf[:] = 0x5A
        else:
            self.buf = np.full(total, 0x5A, dtype=np.uint8)
        self.nbytes, self.off = nbytes, GUARD
        if page_offset is not None:
            self.off += (page_offset - (self.buf.ctypes.data + GUARD)) % 4096
            assert self.ptr % 4096 == page_offset
        assert self.off >= GUARD and self.off + nbytes + GUARD <= total

    @property
    def ptr(self):
        return self.buf.ctypes.data + self.off

    def payload(self):
        return self.buf[self.off:self.off + self.nbytes]

    def guards_intact(self):
        return bool((self.buf[:self.off] == 0x5A).all() and (self.buf[self.off + self.nbytes:] == 0x5A).all())


def host_run(nbytes, dest):
    """mmcmc_mh_discrete_run of a fresh producer into the caller-owned `dest`, through the library's copy"""
    from mini_mcmc_amd import _lib as L

    h = producer(nbytes)
    st = L.lib().mmcmc_mh_discrete_run(h._h, SHAPES[nbytes][1], N_DISCARD, C.c_void_p(dest.ptr), 0, None)
    L.check(st, "mmcmc_mh_discrete_run")


_references = {}


def reference(nbytes):
    """the same run into a torch device tensor, fetched by torch's own .cpu(): uint8 [nbytes]; computed once, read-only"""
    if nbytes not in _references:
        t = producer(nbytes).run(SHAPES[nbytes][1], N_DISCARD, to="torch")
        ref = t.cpu().numpy().reshape(-1).view(np.uint8)
        assert ref.size == nbytes
        values = ref.view(np.int32)
        assert values.min() >= 0 and values.max() > values.min()  # a sample, not a buffer of zeros
        ref.setflags(write=False)
        _references[nbytes] = ref
    return _references[nbytes]


@pytest.fixture(scope="module", autouse=True)
def _drop_references():
    yield
    _references.clear()


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a).reshape(-1).view(np.uint8), np.ascontiguousarray(b).reshape(-1).view(np.uint8)
    if a.size != b.size:
        return False
    if np.array_equal(a, b):
        return True
    bad = np.flatnonzero(a != b)
    print(f"{bad.size} of {a.size} bytes differ, the first at {bad[0]}, the last at {bad[-1]}")
    return False


@pytest.mark.gpu
@pytest.mark.parametrize("nbytes", list(SHAPES), ids=_name)
def test_byte_counts_at_every_chunk_and_ring_edge(nbytes):
    dest = Dest(nbytes)
    host_run(nbytes, dest)
    assert same_bytes(dest.payload(), reference(nbytes))
    assert dest.guards_intact()
    if nbytes not in (32 * MiB + 4, 40 * MiB + 4100):  # those two are used again below
        _references.pop(nbytes, None)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["page_aligned", "four_past_a_page", "pinned"])
def test_destination_kinds(kind):
    nbytes = 40 * MiB + 4100
    dest = Dest(nbytes, page_offset={"page_aligned": 0, "four_past_a_page": 4, "pinned": None}[kind], pinned=kind == "pinned")
    host_run(nbytes, dest)
    assert same_bytes(dest.payload(), reference(nbytes))
    assert dest.guards_intact()


def _callers():
    """name -> (host result through the library, the twin's device result through torch)"""
    from mini_mcmc_amd.core import init_with_seed
    from mini_mcmc_amd.distributions import Gaussian2D, IsotropicGaussian, RosenbrockND, StandardNormal
    from mini_mcmc_amd.gibbs import GibbsSampler, MixtureConditional
    from mini_mcmc_amd.group import HMCGroup
    from mini_mcmc_amd.hmc import HMC
    from mini_mcmc_amd.metropolis_hastings import MetropolisHastings
    from mini_mcmc_amd.nuts import NUTS

    g2 = Gaussian2D([0.0, 1.0], [[4.0, 2.0], [2.0, 3.0]])

    def mh():
        return MetropolisHastings(g2, IsotropicGaussian(1.0), init_with_seed(1031, 2, 42, np.float32)).seed(11)

    def hmc64():
        return HMC(RosenbrockND(3), init_with_seed(701, 3, 42, np.float64), 0.032, 10).set_seed(42)

    def nuts():
        return NUTS(StandardNormal(3), init_with_seed(7001, 3, 5) * 0.5, 0.8, mode=0).set_seed(9)

    def gibbs():
        return GibbsSampler(MixtureConditional(-2.0, 1.0, 3.0, 1.5, 0.5), init_with_seed(1031, 2, 42)).set_seed(5)

    init3 = init_with_seed(3001, 3, 42, np.float32)
    return {
        "mh_f32": lambda: (mh().run(1019, 5), mh().run(1019, 5, to="torch")),
        "hmc_f64": lambda: (hmc64().run(503, 4), hmc64().run(503, 4, to="torch")),
        "nuts": lambda: (nuts().run(101, 10), nuts().run(101, 10, to="torch")),
        "mh_integer_state": lambda: (producer(8 * MiB + 4).run(5419, N_DISCARD), producer(8 * MiB + 4).run(5419, N_DISCARD, to="torch")),
        "gibbs": lambda: (gibbs().run(509, 7), gibbs().run(509, 7, to="torch")),
        "mh_run_progress": lambda: (mh().run_progress(1019, 5)[0], mh().run_progress(1019, 5, to="torch")[0]),
        # three shards of more than a chunk each, queued on the one stager of device 0
        "hmc_group_three_shards": lambda: (HMCGroup(RosenbrockND(3), init3, 0.032, 10, devices=[0, 0, 0]).set_seed(42).run(701, 9),
                                           HMC(RosenbrockND(3), init3, 0.032, 10).set_seed(42).run(701, 9, to="torch")),
    }


@pytest.mark.gpu
@pytest.mark.parametrize("caller", ["mh_f32", "hmc_f64", "nuts", "mh_integer_state", "gibbs", "mh_run_progress", "hmc_group_three_shards"])
def test_every_caller_above_one_chunk_with_a_ragged_tail(caller):
    host, device = _callers()[caller]()
    shard = host.nbytes // 3 if caller == "hmc_group_three_shards" else host.nbytes
    assert shard > 8 * MiB and host.nbytes % 4096 != 0 and shard % 4096 != 0
    assert isinstance(host, np.ndarray) and tuple(host.shape) == tuple(device.shape)
    twin = device.cpu().numpy()
    assert twin.dtype == host.dtype and np.unique(twin.reshape(-1)[:4096]).size > 1
    assert same_bytes(host, twin)


@pytest.mark.gpu
def test_three_copies_in_flight_together():
    nbytes = 40 * MiB + 4100
    ref = reference(nbytes)
    dests = [Dest(nbytes) for _ in range(3)]
    start = threading.Barrier(3)
    errors = []

    def one(dest):
        try:
            start.wait(timeout=60)
            host_run(nbytes, dest)
        except BaseException as e:  # noqa: BLE001 -- reported below
            errors.append(e)

    threads = [threading.Thread(target=one, args=(d,)) for d in dests]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for d in dests:
        assert same_bytes(d.payload(), ref) and d.guards_intact()


@pytest.mark.gpu
def test_copy_thread_counts_in_fresh_processes():
    """k usable CPUs: 1 the plain copy, 2 one copy thread, 6 three, 16 eight (csrc/mm_hostcopy_plan.h: mm_hostcopy_threads)"""
    rows = [32 * MiB + 4, 40 * MiB + 4100]
    want = {b: hashlib.sha256(reference(b)).hexdigest() for b in rows}
    available = len(os.sched_getaffinity(0))
    for k in sorted({1, 2, 6, min(16, available)}):
        r = subprocess.run([sys.executable, CHILD, str(k)] + [str(b) for b in rows], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, f"hostcopy_child {k} ended with {r.returncode}: {r.stdout[-1000:]} {r.stderr[-3000:]}"
        lines = [ln.split() for ln in r.stdout.splitlines() if ln.strip()]
        assert [int(ln[0]) for ln in lines] == rows, r.stdout[-1000:]
        for nbytes, cpus, sha, intact in lines:
            assert int(cpus) == min(k, available), (k, cpus)
            assert sha == want[int(nbytes)], f"{k} CPUs, {nbytes} bytes: the host result differs from torch's copy of the twin"
            assert intact == "1", f"{k} CPUs, {nbytes} bytes: bytes written beside the destination"
