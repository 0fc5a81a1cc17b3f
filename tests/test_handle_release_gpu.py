"""What a handle holds on the device, counted by the library itself: sda_debug_live_device_buffers (include/sda_hip_debug.h, the
test library only) is the number of live device buffers the handles allocated for themselves and their bytes - the library's own
books, so another process allocating on the same GPU does not move them.  For every handle type: take the count, create the handle,
run its entry points once at a small valid shape, run them a second time (a live handle grows its buffers, it does not pile them
up: the buffer count must not move), free the handle, and both counters must be back where they were.  Memory the caller owns
(sda_amd.device: sda_dev_malloc) is not counted.

Only differences are compared, as signed numbers: the Python mirror frees a handle through whichever of the two libraries is active
at that moment, so in a process that ran other tests the test library may have freed handles the release library created, and its
absolute figures mean nothing."""
import ctypes as C
import gc

import numpy as np
import pytest

import reveal_check_cases as vc
import reveal_erasure_cases as ec
from conftest import use_test_hooks

pytestmark = pytest.mark.gpu
P, K, T, N, W2, W3 = vc.SCHEMES["k3_62"]
DIM = 10


def live(lib):
    buffers, nbytes = C.c_size_t(), C.c_size_t()
    assert lib.sda_debug_live_device_buffers(C.byref(buffers), C.byref(nbytes)) == 0
    return buffers.value, nbytes.value


def moved(now, then):
    """now - then per counter, as signed 64-bit numbers"""
    return tuple(((a - b + (1 << 63)) % (1 << 64)) - (1 << 63) for a, b in zip(now, then))


def _keys(seed):
    from oracle import sealedbox_oracle as so
    sk = bytes(np.random.default_rng(seed).integers(0, 256, 32, dtype=np.uint8))
    return so.x25519_base(sk), sk


def _secrets(rows=1):
    return np.random.default_rng(81).integers(0, P, size=(rows, DIM), dtype=np.int64)


# ---- one function per handle type: (the handle, a callable that runs its entry points once) --------------------------------------------
def share_generator(crypto):
    h = crypto.ShareGenerator(crypto.PackedShamir(K, N, T, P, W2, W3))
    h.set_drbg_key(bytes(range(32)))
    return h, lambda: h.generate(_secrets()[0])


def share_combiner(crypto):
    from sda_amd.device import DeviceBuffer
    h = crypto.ShareCombiner(crypto.PackedShamir(K, N, T, P, W2, W3))
    shares = _secrets(3)
    d_shares, d_out = DeviceBuffer.from_numpy(shares), DeviceBuffer(DIM)

    def run():
        assert np.array_equal(h.combine(list(shares)), (shares.astype(object).sum(axis=0) % P).astype(np.int64))
        h.begin_dev(1, DIM)
        h.update_dev(d_shares.ptr, 3 * DIM, 3, DIM)
        h.finish_dev(d_out.ptr)
        h.begin(DIM)
        h.update(shares)
        h.finish()
    return h, run


def secret_reconstructor(crypto):
    """reconstruct, a plain job, a checked job ended each of the three ways, reconstruct_erasures with an erased list"""
    from sda_amd.device import DeviceBuffer, DeviceBytes
    case, b = ec.BY_NAME[ec.E2E], ec.build(ec.E2E)
    h = crypto.SecretReconstructor(crypto.PackedShamir(K, N, T, P, W2, W3), case.dim)
    pos, L = b.rows.shape
    pairs = [(i, r) for i, r in zip(case.indices, b.rows)]
    d_rows = DeviceBuffer.from_numpy(np.ascontiguousarray(b.rows))
    d_out, d_report = DeviceBuffer(case.dim + 1), DeviceBuffer(ec.HEAD + pos)
    d_ok = DeviceBytes.from_bytes(np.ascontiguousarray(ec.ok_words(case), dtype="<u4").tobytes())

    def run():
        h.reconstruct(pairs[:T + K])
        h.begin_dev(case.indices, pos, L)
        h.update_dev(0, d_rows.ptr, pos, L)
        h.finish_dev(d_out.ptr, case.dim)
        for end in (lambda: h.finish_checked_dev(d_out.ptr, case.dim, d_report.ptr, True),
                    lambda: h.finish_decoded_dev(d_out.ptr, case.dim, d_report.ptr, 0, True),
                    lambda: h.finish_erasures_dev(d_ok.ptr, d_out.ptr, case.dim, d_report.ptr, 0, True)):
            h.begin_checked_dev(case.indices, pos, L, case.checks)
            h.update_dev(0, d_rows.ptr, pos, L)
            end()
        erased = [i in case.erased for i in range(pos)]
        vals, dec, f, unrepaired = h.reconstruct_erasures(pairs, erased, checks=case.checks, correct=True)
        assert np.array_equal(vals, b.want) and f == len(case.erased) and not unrepaired
    return h, run


def secret_masker(crypto):
    h = crypto.SecretMasker(crypto.Full(P))
    h.set_drbg_key(bytes(range(32)))
    return h, lambda: h.mask(_secrets()[0])


def mask_combiner(crypto):
    h = crypto.MaskCombiner(crypto.Full(P))
    return h, lambda: h.combine(list(_secrets(3)))


def secret_unmasker(crypto):
    h = crypto.SecretUnmasker(crypto.Full(P))
    return h, lambda: h.unmask((_secrets()[0], _secrets()[0]))


def varint_codec(crypto):
    h = crypto.VarintCodec()

    def run():
        assert np.array_equal(h.decode(h.encode(_secrets()[0])), _secrets()[0])
    return h, run


def sealed_box(crypto):
    h = crypto.SealedBox()
    pk, sk = _keys(82)

    def run():
        assert h.open(h.seal(b"a clerking result", pk), pk, sk) == b"a clerking result"
    return h, run


HANDLES = (share_generator, share_combiner, secret_reconstructor, secret_masker, mask_combiner, secret_unmasker, varint_codec, sealed_box)


@pytest.mark.parametrize("make", HANDLES, ids=[f.__name__ for f in HANDLES])
def test_a_freed_handle_gives_back_every_buffer_it_took(gpu, make):
    from sda_amd import crypto
    lib = use_test_hooks()
    gc.collect()                                               # handles of earlier tests that nobody holds any more
    before = live(lib)
    handle, run = make(crypto)
    run()
    held = live(lib)
    run()
    again = live(lib)
    handle.close()
    after = live(lib)
    took, left = moved(held, before), moved(after, before)
    print(f"{make.__name__}: took {took} (buffers, bytes), after a second pass {moved(again, before)}, left behind {left}")
    assert took[0] > 0 and took[1] > 0, "the handle took nothing: the count does not see its buffers"
    assert again[0] == held[0], "a second identical call on a live handle changed the number of buffers it holds"
    assert left == (0, 0), f"the freed handle left {left[0]} buffers ({left[1]} bytes) behind"
