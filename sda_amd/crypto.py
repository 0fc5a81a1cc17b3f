"""Host-side mirror of the reference's ``client::crypto`` sharing / masking interface, on top of
the C ABI (include/sda_hip.h).  Same names, argument meaning and error behaviour as the reference:

    CryptoModule.new_share_generator(scheme)         sharing/mod.rs:10-12,35-55
    ShareGenerator.generate(secrets)                 sharing/mod.rs:14-17
    CryptoModule.new_share_combiner(scheme)          sharing/mod.rs:19-21,57-73
    ShareCombiner.combine(shares)                    sharing/mod.rs:23-25
    CryptoModule.new_secret_reconstructor(scheme, d) sharing/mod.rs:27-29,75-96
    SecretReconstructor.reconstruct(indexed_shares)  sharing/mod.rs:31-33
    CryptoModule.new_secret_masker / new_mask_combiner / new_secret_unmasker   masking/mod.rs:9-31

``SdaClientResult`` errors surface as :class:`sda_amd.capi.SdaError` carrying the reference's message;
the masking traits' ``assert!`` panics surface as :class:`AssertionError`.  The only widening of the
interface is the optional ``rand`` argument (the reference draws from OsRng; see sda_hip.h).

Every method runs on the GPU through libsda_hip.so; nothing here computes on share data in Python.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np

from . import capi
from .capi import SdaError, check

Secret = Mask = MaskedSecret = Share = np.int64     # client/src/crypto/mod.rs:33-36


# ---- scheme enums (protocol/src/crypto.rs:43-155) ------------------------------------------------
@dataclass(frozen=True)
class Additive:
    share_count: int
    modulus: int

    def input_size(self): return 1                                   # crypto.rs:120-126
    def output_size(self): return self.share_count                   # crypto.rs:129-135
    def privacy_threshold_(self): return self.share_count - 1        # crypto.rs:138-144
    def reconstruction_threshold(self): return self.share_count      # crypto.rs:147-153

    def _c(self):
        return capi.SharingScheme(capi.SHARING_ADDITIVE, self.share_count, self.modulus, 0, 0, 0, 0)


@dataclass(frozen=True)
class PackedShamir:
    secret_count: int
    share_count: int
    privacy_threshold: int
    prime_modulus: int
    omega_secrets: int
    omega_shares: int

    def input_size(self): return self.secret_count
    def output_size(self): return self.share_count
    def privacy_threshold_(self): return self.privacy_threshold
    def reconstruction_threshold(self): return self.privacy_threshold + self.secret_count

    def _c(self):
        return capi.SharingScheme(capi.SHARING_PACKED_SHAMIR, self.share_count, self.prime_modulus,
                                  self.secret_count, self.privacy_threshold, self.omega_secrets,
                                  self.omega_shares)


LinearSecretSharingScheme = Union[Additive, PackedShamir]


@dataclass(frozen=True)
class NoMask:                       # LinearMaskingScheme::None
    def has_mask(self): return False
    def _c(self): return capi.MaskingScheme(capi.MASKING_NONE, 0, 0, 0)


@dataclass(frozen=True)
class Full:
    modulus: int
    def has_mask(self): return True
    def _c(self): return capi.MaskingScheme(capi.MASKING_FULL, self.modulus, 0, 0)


@dataclass(frozen=True)
class ChaCha:
    modulus: int
    dimension: int
    seed_bitsize: int
    def has_mask(self): return True
    def _c(self): return capi.MaskingScheme(capi.MASKING_CHACHA, self.modulus, self.dimension, self.seed_bitsize)


LinearMaskingScheme = Union[NoMask, Full, ChaCha]


# ---- helpers ------------------------------------------------------------------------------------------
def _vec(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.int64).reshape(-1)


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(capi.c_i64p)


def _index_array(indices: Optional[Sequence[int]]):
    """clerk indices as a size_t array for the C ABI (never of length 0); None stays None"""
    return None if indices is None else (C.c_size_t * max(len(indices), 1))(*[int(i) for i in indices])


def _rows(vectors: Sequence) -> Tuple[List[np.ndarray], C.Array, C.Array]:
    if isinstance(vectors, np.ndarray) and vectors.ndim == 2 and vectors.dtype == np.int64 and vectors.shape[0] > 0 \
            and vectors.strides[1] == 8:
        # a matrix: row pointers by arithmetic instead of one ctypes object per row (thousands of seeds / vectors)
        n = vectors.shape[0]
        addr = (vectors.ctypes.data + np.arange(n, dtype=np.uint64) * np.uint64(vectors.strides[0])).astype(np.uint64)
        lens_np = np.full(n, vectors.shape[1], dtype=np.uint64)
        ptrs = C.cast(addr.ctypes.data_as(C.POINTER(C.c_uint64)), C.POINTER(capi.c_i64p))
        lens = C.cast(lens_np.ctypes.data_as(C.POINTER(C.c_uint64)), C.POINTER(C.c_size_t))
        rows = _MatrixRows(vectors, addr, lens_np)
        return rows, ptrs, lens
    arrs = [_vec(v) for v in vectors]
    ptrs = (capi.c_i64p * max(len(arrs), 1))(*[_ptr(a) for a in arrs])
    lens = (C.c_size_t * max(len(arrs), 1))(*[a.size for a in arrs])
    return arrs, ptrs, lens


class _MatrixRows(list):
    """keeps the matrix and the pointer/length arrays alive; len() = rows, [0].size = columns"""

    def __init__(self, matrix, addr, lens):
        super().__init__(matrix)
        self._keep = (matrix, addr, lens)


def _check_mask(status: int) -> None:
    """masking traits are infallible in the reference and panic on assert! - mirror as AssertionError"""
    if status == capi.ERR_ASSERTION:
        raise AssertionError(capi.load().sda_last_error().decode())
    check(status)


CANONICAL, RUST_SIGNED = 0, 1          # enum sda_value_mode


class _Handle:
    _free = None
    _value_mode = None                  # name of the C setter, for the six trait handles

    def __init__(self):
        self._h = C.c_void_p()
        self._lib = capi.load()

    def set_value_mode(self, mode) -> "_Handle":
        """CANONICAL (default): residues in [0, q).  RUST_SIGNED: the reference's own representatives, bit for bit
        (Rust's truncated `%`: values in (-q, q), history-dependent signs) - additive sharing, the combiner, the masks."""
        mode = {"canonical": CANONICAL, "rust_signed": RUST_SIGNED}.get(mode, mode)
        check(getattr(self._lib, self._value_mode)(self._h, int(mode)))
        return self

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            getattr(self._lib, self._free)(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- sharing ----------------------------------------------------------------------------------------------
class ShareGenerator(_Handle):
    """sharing/mod.rs:14-17; impl batched.rs:18-53 over additive.rs / packed_shamir.rs."""
    _free = "sda_share_generator_free"
    _value_mode = "sda_share_generator_set_value_mode"

    def __init__(self, scheme: LinearSecretSharingScheme):
        super().__init__()
        self.scheme = scheme
        cs = scheme._c()
        check(self._lib.sda_share_generator_new(C.byref(cs), C.byref(self._h)))

    def set_drbg_key(self, key: bytes):
        """TEST / BENCH ONLY: deterministic mode (the caller's stream ids select the CSPRNG streams)"""
        if len(key) != 32:
            raise ValueError("the CSPRNG key is exactly 32 bytes")
        check(self._lib.sda_share_generator_set_drbg_key(self._h, (C.c_uint8 * 32)(*key)))

    def set_drbg_master_key(self, key: bytes):
        """TEST ONLY: fixed master key, per-call key derivation stays on"""
        if len(key) != 32:
            raise ValueError("the CSPRNG key is exactly 32 bytes")
        check(self._lib.sda_share_generator_set_drbg_master_key(self._h, (C.c_uint8 * 32)(*key)))

    def set_drbg_rounds(self, rounds: int):
        check(self._lib.sda_share_generator_set_drbg_rounds(self._h, rounds))

    SHARE_MAP_TSS_NODES, SHARE_MAP_SYSTEMATIC = 0, 1

    def csprng_share_map(self) -> int:
        """the parametrisation calls WITHOUT injected randomness use (include/sda_hip.h, "CSPRNG share map"): 1 = the t draws
        of a batch are its shares 0..t-1, 0 = tss's (draws are the values at omega_secrets^(k+1..k+t))"""
        return int(self._lib.sda_share_generator_csprng_share_map(self._h))

    def set_csprng_share_map(self, which: int):
        check(self._lib.sda_share_generator_set_csprng_share_map(self._h, which))

    def path_name(self) -> str:
        """the kernel family the library selected for this scheme ("l31", "fft+ngemm", ... - sda_amd/csrc/path_select.hpp)"""
        return self._lib.sda_share_generator_path_name(self._h).decode()

    def batch_count(self, length: int) -> int:
        return int(self._lib.sda_share_generator_batch_count(self._h, length))

    def rand_count(self, length: int) -> int:
        return int(self._lib.sda_share_generator_rand_count(self._h, length))

    def generate(self, secrets, rand=None) -> np.ndarray:
        """-> int64 array [share_count][batches], row j = the shares for clerk j (batched.rs:46-48)."""
        s = _vec(secrets)
        n = int(self._lib.sda_share_generator_share_count(self._h))
        B = self.batch_count(s.size)
        out = np.empty((n, B), dtype=np.int64)
        if rand is None:
            rp, rl = None, 0
        else:
            r = _vec(rand)
            rp, rl = _ptr(r), r.size
        check(self._lib.sda_share_generator_generate(self._h, _ptr(s), s.size, rp, rl, _ptr(out), out.size))
        return out

    def generate_batch_dev(self, d_secrets: int, participants: int, length: int, secrets_stride: int,
                           d_out: int, out_stride_participant: int, out_stride_clerk: int,
                           first_participant: int = 0, d_rand: int = 0, rand_stride: int = 0, stream: int = 0):
        check(self._lib.sda_share_generator_generate_batch_dev(
            self._h, d_secrets, participants, length, secrets_stride, d_rand or None, rand_stride,
            first_participant, d_out, out_stride_participant, out_stride_clerk, stream or None))

    def generate_sealed_rows_dev(self, codec: "VarintCodec", box: "SealedBox", pks: Sequence[bytes], d_secrets: int, participants: int,
                                 length: int, secrets_stride: int, d_boxes: int, slot_bytes: int, d_row_bytes: int,
                                 first_participant: int = 0, esk: Optional[bytes] = None, stream: int = 0) -> None:
        """secrets -> the sealed rows of every clerking job in one call (participate.rs:75-101); no share reaches device memory.
        pks: the share_count clerk keys in clerk order.  Row c * participants + p = clerk c's box for participant p, at
        d_boxes + row * slot_bytes, its length (0: refused) in d_row_bytes[row].  Device CSPRNG, canonical values, additive or
        packed Shamir with secret_count + privacy_threshold <= 32."""
        allpk = b"".join(pks)
        assert len(allpk) == 32 * len(pks) and (esk is None or len(esk) == 32 * len(pks) * participants)
        n = int(self._lib.sda_share_generator_share_count(self._h))
        if len(pks) != n:
            raise ValueError(f"one key per clerk: {n} keys, got {len(pks)}")
        check(self._lib.sda_share_generator_generate_sealed_rows_dev(
            self._h, codec._h, box._h, allpk, esk, d_secrets or None, participants, length, secrets_stride, first_participant,
            d_boxes, slot_bytes, d_row_bytes, stream or None))

    def generate_combine_dev(self, combiner: "ShareCombiner", d_secrets: int, participants: int, length: int,
                             secrets_stride: int, d_out: int, out_stride_participant: int, out_stride_clerk: int,
                             d_prev: int = 0, prev_participants: int = 0, first_participant: int = 0, stream: int = 0):
        """software-pipelined step: generate this tile while the previous tile (d_prev) is summed into `combiner`"""
        check(self._lib.sda_share_generator_generate_combine_dev(
            self._h, combiner._h, d_secrets or None, participants, length, secrets_stride, first_participant,
            d_out or None, out_stride_participant, out_stride_clerk, d_prev or None, prev_participants, stream or None))


class ShareCombiner(_Handle):
    """sharing/mod.rs:23-25; impl combiner.rs:15-29."""
    _free = "sda_share_combiner_free"
    _value_mode = "sda_share_combiner_set_value_mode"

    def __init__(self, scheme: LinearSecretSharingScheme):
        super().__init__()
        self.scheme = scheme
        cs = scheme._c()
        check(self._lib.sda_share_combiner_new(C.byref(cs), C.byref(self._h)))

    def combine(self, shares: Sequence) -> np.ndarray:
        arrs, ptrs, lens = _rows(shares)
        cap = arrs[0].size if arrs else 0
        out = np.empty(max(cap, 1), dtype=np.int64)
        n_out = C.c_size_t()
        check(self._lib.sda_share_combiner_combine(self._h, ptrs, lens, len(arrs), _ptr(out), cap, C.byref(n_out)))
        return out[:n_out.value].copy()

    # streaming / accumulating form (fixes the FIXME at client/src/clerk.rs:71-72)
    def begin(self, dimension: int):
        check(self._lib.sda_share_combiner_begin(self._h, dimension))
        self._dimension = dimension

    def update(self, tile) -> None:
        t = np.ascontiguousarray(tile, dtype=np.int64)
        assert t.ndim == 2
        check(self._lib.sda_share_combiner_update(self._h, _ptr(t), t.shape[0], t.shape[1]))

    def finish(self, dimension: Optional[int] = None) -> np.ndarray:
        """the dimension is the one given to begin(); an argument is accepted only if it agrees"""
        have = getattr(self, "_dimension", None)
        if have is None:
            raise SdaError(capi.ERR_STATE, "finish before begin")
        if dimension is not None and dimension != have:
            raise ValueError(f"finish({dimension}) on a combiner begun with dimension {have}")
        out = np.empty(max(have, 1), dtype=np.int64)
        check(self._lib.sda_share_combiner_finish(self._h, _ptr(out)))
        return out[:have]

    def update_encoded(self, codec: "VarintCodec", raw: bytes) -> None:
        """one participant's wire-format share vector (the opened sealed-box payload, sodium.rs:83-89)"""
        b = np.frombuffer(raw, dtype=np.uint8)
        check(self._lib.sda_share_combiner_update_varint(self._h, codec._h, b.ctypes.data_as(capi.c_u8p), b.size))

    def update_encoded_dev(self, codec: "VarintCodec", d_bytes: int, n_bytes: int, d_row_offsets: int, rows: int,
                           d_status: int, stream: int = 0) -> None:
        check(self._lib.sda_share_combiner_update_varint_dev(self._h, codec._h, d_bytes, n_bytes, d_row_offsets or None,
                                                             rows, d_status, stream or None))

    def update_encoded_rows_dev(self, codec: "VarintCodec", d_bytes: int, slot_bytes: int, d_row_bytes: int, rows: int,
                                d_status: int, stream: int = 0) -> None:
        check(self._lib.sda_share_combiner_update_varint_rows_dev(self._h, codec._h, d_bytes, slot_bytes, d_row_bytes,
                                                                  rows, d_status, stream or None))

    def update_sealed_rows_dev(self, codec: "VarintCodec", box: "SealedBox", pk: bytes, sk: bytes, d_boxes: int,
                               slot_bytes: int, d_row_bytes: int, rows: int, max_box_bytes: int, d_status: int, d_ok: int = 0,
                               stream: int = 0) -> None:
        """rows that are still sealed boxes (the SDAJOBv1 SEALED layout): tags verified, then decrypted, decoded and summed
        in one pass - no plaintext buffer.  *d_status & 16: some box failed, the sums must not be used (sodium.rs:78-80)"""
        check(self._lib.sda_share_combiner_update_sealed_rows_dev(self._h, codec._h, box._h, pk, sk, d_boxes, slot_bytes,
                                                                  d_row_bytes, rows, max_box_bytes, d_ok or None, d_status,
                                                                  stream or None))

    def _sum_sealed_job(self, what: str, blob, pk: bytes, sk: bytes, dimension: int, codec: "VarintCodec", box: "SealedBox") -> int:
        """begin_dev(1, dimension) + update_sealed_rows_dev over an SDAJOBv1 blob of sealed boxes, its failures raised as the
        reference's; returns the number of rows (0: nothing was begun)"""
        from .device import DeviceBuffer, DeviceBytes
        job = _parse_sealed_job(what, blob)
        L = job.layout
        if L.rows == 0:
            return 0
        d_job = DeviceBytes.from_bytes(job.blob)
        d_status = DeviceBuffer(1).zero()
        self.begin_dev(1, dimension)
        self.update_sealed_rows_dev(codec, box, pk, sk, d_job.ptr + L.payload_offset, L.slot_bytes, d_job.ptr + L.lengths_offset,
                                    L.rows, L.slot_bytes, d_status.ptr)
        _raise_sealed_status(int(d_status.to_numpy()[0]))
        return L.rows

    def combine_sealed_job(self, blob, pk: bytes, sk: bytes, dimension: int) -> np.ndarray:
        """clerk.rs:78-86 for an SDAJOBv1 blob of sealed boxes: open every encryption, decode it, sum the share vectors.
        One bad box fails the job ("Sodium decryption failure"), so does a payload that does not hold `dimension` shares
        ("Wrong dimension")."""
        from .device import DeviceBuffer
        if self._sum_sealed_job("combine_sealed_job", blob, pk, sk, dimension, VarintCodec(), SealedBox()) == 0:
            return np.zeros(0, dtype=np.int64)                       # combiner.rs:17
        d_sums = DeviceBuffer(max(dimension, 1))
        self.finish_dev(d_sums.ptr)
        return d_sums.to_numpy()[:dimension].copy()

    def finish_sealed_rows_dev(self, codec: "VarintCodec", box: "SealedBox", recipient_pk: bytes, d_boxes: int, slot_bytes: int,
                               d_row_bytes: int, esk: Optional[bytes] = None, stream: int = 0) -> None:
        """the clerk's last step (clerk.rs:84-100) on the device job: job j's sums reduced, varint encoded and sealed to the
        recipient into d_boxes + j * slot_bytes, d_row_bytes[j] = payload + 48 (0: refused) - every row split over the whole
        chip, no plaintext result and no wire buffer.  The job stays valid.  esk injects jobs*32 bytes (tests only)."""
        assert len(recipient_pk) == 32
        check(self._lib.sda_share_combiner_finish_sealed_rows_dev(self._h, codec._h, box._h, recipient_pk, esk, d_boxes, slot_bytes,
                                                                  d_row_bytes, stream or None))

    def clerk_sealed_job(self, blob, pk: bytes, sk: bytes, recipient_pk: bytes, dimension: int, esk: Optional[bytes] = None) -> bytes:
        """process_clerking_job (clerk.rs:71-100) for an SDAJOBv1 blob of sealed boxes: combine_sealed_job, then the sums sealed
        to the recipient - the clerking result's encryption.  Neither a share nor a sum is written to device memory in plain.
        A job without rows gives the encryption of the empty vector (combiner.rs:17)."""
        from .device import DeviceBuffer, DeviceBytes
        assert esk is None or len(esk) == 32
        codec, box = VarintCodec(), SealedBox()
        if self._sum_sealed_job("clerk_sealed_job", blob, pk, sk, dimension, codec, box) == 0:
            dimension = 0
            self.begin_dev(1, 0)
        slot = int(self._lib.sda_varint_slot_size(dimension)) + 48
        d_box, d_len = DeviceBytes(slot), DeviceBuffer(1).zero()
        self.finish_sealed_rows_dev(codec, box, recipient_pk, d_box.ptr, slot, d_len.ptr, esk)
        n = int(d_len.to_numpy()[0])
        if n == 0:
            raise SdaError(capi.ERR_INVALID_ARGUMENT, "sealing refused: the recipient public key is a small-order point")
        return d_box.to_bytes()[:n]

    def set_residency(self, max_workgroups_per_cu: int) -> None:
        check(self._lib.sda_share_combiner_set_residency(self._h, max_workgroups_per_cu))

    def begin_dev(self, jobs: int, dimension: int, stream: int = 0):
        check(self._lib.sda_share_combiner_begin_dev(self._h, jobs, dimension, stream or None))
        self._dimension = dimension if jobs == 1 else None

    def update_dev(self, d_shares: int, job_stride: int, n_rows: int, row_stride: int, stream: int = 0):
        check(self._lib.sda_share_combiner_update_dev(self._h, d_shares, job_stride, n_rows, row_stride, stream or None))

    def finish_dev(self, d_out: int, stream: int = 0):
        check(self._lib.sda_share_combiner_finish_dev(self._h, d_out, stream or None))


def _parse_sealed_job(what: str, blob) -> "JobContainer":
    """an SDAJOBv1 blob that must hold sealed boxes"""
    job = JobContainer.parse(bytes(blob))
    if job.layout.payload_kind != capi.JOB_SEALED:
        raise SdaError(capi.ERR_INVALID_ARGUMENT, f"{what} needs a job of sealed boxes (payload kind SEALED)")
    return job


def _raise_sealed_status(status: int) -> None:
    """the status word of a sealed update as the reference's errors, in their order of precedence"""
    status &= 0xFFFFFFFF
    if status & 16:
        raise SdaError(capi.ERR_SODIUM_DECRYPTION, "Sodium decryption failure")        # sodium.rs:80
    if status & 2:
        raise SdaError(capi.ERR_WRONG_DIMENSION, "Wrong dimension")                    # combiner.rs:21
    if status:
        raise SdaError(capi.ERR_INVALID_ARGUMENT, f"malformed varint stream (status {status})")


class RevealCheck(NamedTuple):
    """the report of a checked reconstruction: batches with a non-zero syndrome, those located to exactly one position, those
    corrected, the first bad batch (None: none) and, per POSITION of the index set, the batches that blame it"""
    bad: int
    located: int
    corrected: int
    first_bad: Optional[int]
    blame: Tuple[int, ...]
    HEAD = 4                         # report words before the blame

    @property
    def clean(self) -> bool:
        return self.bad == 0

    @classmethod
    def from_words(cls, words: Sequence[int]) -> "RevealCheck":
        w = [int(x) & 0xFFFFFFFFFFFFFFFF for x in words]
        return cls(w[0], w[1], w[2], None if w[3] == 0xFFFFFFFFFFFFFFFF else w[3], tuple(w[cls.HEAD:]))


class RevealDecode(NamedTuple):
    """the report of a decoded reconstruction: batches with a non-zero syndrome, those decoded (with 1 .. 8 positions), those
    corrected, the first bad and the first UNDECODED batch (None: none), the largest number of positions a batch was decoded with,
    by_count[nu - 1] = batches decoded with exactly nu positions and, per POSITION of the index set, the batches that blame it"""
    bad: int
    decoded: int
    corrected: int
    first_bad: Optional[int]
    first_undecoded: Optional[int]
    most: int
    by_count: Tuple[int, ...]
    blame: Tuple[int, ...]
    HEAD = 16                        # report words before the blame

    @property
    def clean(self) -> bool:
        return self.bad == 0

    @property
    def undecoded(self) -> int:
        return self.bad - self.decoded

    @classmethod
    def from_words(cls, words: Sequence[int]) -> "RevealDecode":
        w = [int(x) & 0xFFFFFFFFFFFFFFFF for x in words]
        none = 0xFFFFFFFFFFFFFFFF
        return cls(w[0], w[1], w[2], None if w[3] == none else w[3], None if w[4] == none else w[4], w[5], tuple(w[8:cls.HEAD]), tuple(w[cls.HEAD:]))


class SecretReconstructor(_Handle):
    """sharing/mod.rs:31-33; impl additive.rs:55-73 | batched.rs:68-97 + packed_shamir.rs:73-77."""
    _free = "sda_secret_reconstructor_free"
    _value_mode = "sda_secret_reconstructor_set_value_mode"

    def __init__(self, scheme: LinearSecretSharingScheme, dimension: int):
        super().__init__()
        self.scheme = scheme
        self.dimension = dimension
        cs = scheme._c()
        check(self._lib.sda_secret_reconstructor_new(C.byref(cs), dimension, C.byref(self._h)))

    def reconstruct(self, indexed_shares: Sequence[Tuple[int, Sequence]]) -> np.ndarray:
        arrs, ptrs, lens = _rows([v for _, v in indexed_shares])
        cidx = _index_array([i for i, _ in indexed_shares])
        cap = max(self.dimension, arrs[0].size if arrs else 0)
        out = np.empty(max(cap, 1), dtype=np.int64)
        n_out = C.c_size_t()
        check(self._lib.sda_secret_reconstructor_reconstruct(self._h, cidx, ptrs, lens, len(arrs), _ptr(out), cap,
                                                             C.byref(n_out)))
        return out[:n_out.value].copy()

    def reconstruct_dev(self, indices: Sequence[int], d_shares: int, row_len: int, row_stride: int, d_out: int,
                        out_cap: int, stream: int = 0) -> int:
        n_out = C.c_size_t()
        check(self._lib.sda_secret_reconstructor_reconstruct_dev(self._h, _index_array(indices), len(indices), d_shares, row_len,
                                                                 row_stride, d_out, out_cap, C.byref(n_out),
                                                                 stream or None))
        return n_out.value

    # streaming device form (receive.rs:120-146 with the clerking results in HBM): no update synchronises or copies to the host
    def begin_dev(self, indices: Optional[Sequence[int]], n_rows: int, row_len: int, stream: int = 0) -> None:
        """declares the job: indices[i] is the clerk index of position i (Additive: None), every row holds row_len values"""
        check(self._lib.sda_secret_reconstructor_begin_dev(self._h, self._job_indices(indices, n_rows), n_rows, row_len, stream or None))

    def _job_indices(self, indices: Optional[Sequence[int]], n_rows: int):
        if indices is not None and len(indices) != n_rows:
            raise SdaError(capi.ERR_INVALID_ARGUMENT, f"{len(indices)} indices for {n_rows} rows")
        return _index_array(indices)

    def update_dev(self, first_pos: int, d_shares: int, rows: int, row_stride: int, stream: int = 0) -> None:
        """decoded rows in HBM for positions first_pos .. first_pos + rows - 1"""
        check(self._lib.sda_secret_reconstructor_update_dev(self._h, first_pos, d_shares or None, rows, row_stride, stream or None))

    def update_sealed_rows_dev(self, codec: "VarintCodec", box: "SealedBox", pk: bytes, sk: bytes, first_pos: int, d_boxes: int,
                               slot_bytes: int, d_row_bytes: int, rows: int, max_box_bytes: int, d_status: int, d_ok: int = 0,
                               stream: int = 0) -> None:
        """the same positions from clerking results that are still sealed boxes (the SDAJOBv1 SEALED layout).
        *d_status & 16: some box failed, the result must not be used (sodium.rs:78-80)"""
        check(self._lib.sda_secret_reconstructor_update_sealed_rows_dev(self._h, codec._h if codec else None,
                                                                        box._h if box else None, pk, sk, first_pos,
                                                                        d_boxes or None, slot_bytes, d_row_bytes or None, rows,
                                                                        max_box_bytes, d_ok or None, d_status or None,
                                                                        stream or None))

    def finish_dev(self, d_out: int, out_cap: int, stream: int = 0) -> None:
        check(self._lib.sda_secret_reconstructor_finish_dev(self._h, d_out or None, out_cap, stream or None))

    # the checked job (PackedShamir): the surplus rows as parity checks - which clerking result disagrees with the others
    def default_checks(self, n_rows: int) -> int:
        """min(n_rows - (t + k), 4): what checks=None asks for"""
        return min(n_rows - (self.scheme.privacy_threshold + self.scheme.secret_count), 4)

    def begin_checked_dev(self, indices: Sequence[int], n_rows: int, row_len: int, checks: int, stream: int = 0) -> None:
        """begin_dev with `checks` parity columns behind the k secret columns; update_dev / update_sealed_rows_dev feed it"""
        cidx = self._job_indices(indices, n_rows)
        check(self._lib.sda_secret_reconstructor_begin_checked_dev(self._h, cidx, n_rows, row_len, checks, stream or None))

    def finish_checked_dev(self, d_out: int, out_cap: int, d_report: int, correct: bool = False, stream: int = 0) -> None:
        """folds, tests the syndromes, locates, corrects on request; d_report: 4 + n_rows device words (RevealCheck.from_words).
        Nothing synchronises or reaches the host"""
        check(self._lib.sda_secret_reconstructor_finish_checked_dev(self._h, capi.CHECK_CORRECT if correct else capi.CHECK_REPORT,
                                                                    d_out or None, out_cap, d_report or None, stream or None))

    def reconstruct_checked(self, indexed_shares: Sequence[Tuple[int, Sequence]], checks: Optional[int] = None,
                            correct: bool = False) -> Tuple[np.ndarray, "RevealCheck"]:
        """reconstruct() that also says whether the rows agree: (values, RevealCheck)"""
        return self._reconstruct_with_checks(RevealCheck, indexed_shares, checks, 0, correct)

    def _reconstruct_with_checks(self, kind, indexed_shares, checks: Optional[int], max_errors: int, correct: bool):
        """reconstruct_checked (kind RevealCheck; max_errors is not read) and reconstruct_decoded (RevealDecode)"""
        arrs, ptrs, lens = _rows([v for _, v in indexed_shares])
        cidx = _index_array([i for i, _ in indexed_shares])
        if checks is None and not isinstance(self.scheme, Additive):
            checks = self.default_checks(len(arrs))
        out = np.empty(max(self.dimension, 1), dtype=np.int64)
        report = (C.c_uint64 * (kind.HEAD + len(arrs)))()
        n_out = C.c_size_t()
        head = (self._h, cidx, ptrs, lens, len(arrs), max(int(checks or 0), 0))
        tail = (capi.CHECK_CORRECT if correct else capi.CHECK_REPORT, _ptr(out), self.dimension, C.byref(n_out), report)
        if kind is RevealCheck:
            check(self._lib.sda_secret_reconstructor_reconstruct_checked(*head, *tail))
        else:
            check(self._lib.sda_secret_reconstructor_reconstruct_decoded(*head, max_errors, *tail))
        return out[:n_out.value].copy(), kind.from_words(list(report))

    def reconstruct_sealed_job_checked(self, blob, indices: Sequence[int], pk: bytes, sk: bytes, checks: Optional[int] = None,
                                       correct: bool = False) -> Tuple[np.ndarray, "RevealCheck"]:
        """reconstruct_sealed_job with the checks riding along: (values, RevealCheck).  A bad box still fails the reveal
        (sodium.rs:78-80) - the check is for results that open and disagree"""
        return self._reconstruct_sealed_job_with_checks(RevealCheck, "reconstruct_sealed_job_checked", blob, indices, pk, sk, checks, 0, correct)

    def _reconstruct_sealed_job_with_checks(self, kind, name: str, blob, indices, pk, sk, checks, max_errors: int, correct: bool):
        """reconstruct_sealed_job_checked (kind RevealCheck; max_errors is not read) and reconstruct_sealed_job_decoded (RevealDecode)"""
        from .device import DeviceBuffer
        job = _parse_sealed_job(name, blob)
        row_len, n_out = self._sealed_job_shape(None)
        rows = job.layout.rows
        checks = self.default_checks(rows) if checks is None else checks
        # [0]: the status word, [1 .. first): the report, then the output
        first = 1 + kind.HEAD + rows
        d_buf = DeviceBuffer(first + max(n_out, 1)).zero()
        held = self._feed_sealed_job(job, indices, row_len, pk, sk, d_buf.at(0), checks=checks)
        self._finish_with_checks(kind, d_buf.at(first), n_out, d_buf.at(1), max_errors, correct)
        back = d_buf.to_numpy()
        del held
        _raise_sealed_status(int(back[0]))
        return back[first:first + n_out].copy(), kind.from_words(back[1:first].view(np.uint64).tolist())

    def _finish_with_checks(self, kind, d_out: int, out_cap: int, d_report: int, max_errors: int, correct: bool) -> None:
        """finish_checked_dev (kind RevealCheck; max_errors is not read) or finish_decoded_dev (RevealDecode)"""
        if kind is RevealCheck:
            self.finish_checked_dev(d_out, out_cap, d_report, correct)
        else:
            self.finish_decoded_dev(d_out, out_cap, d_report, max_errors, correct)

    # the decoding finish of a checked job: up to floor(checks / 2) disagreeing clerking results per batch, named and repaired
    def finish_decoded_dev(self, d_out: int, out_cap: int, d_report: int, max_errors: int = 0, correct: bool = False,
                           stream: int = 0) -> None:
        """ends a job begun by begin_checked_dev: folds, decodes every bad batch with at most max_errors positions (0:
        floor(checks / 2)), corrects on request; d_report: 16 + n_rows device words (RevealDecode.from_words).  Nothing
        synchronises or reaches the host"""
        check(self._lib.sda_secret_reconstructor_finish_decoded_dev(self._h, max_errors, capi.CHECK_CORRECT if correct else capi.CHECK_REPORT,
                                                                    d_out or None, out_cap, d_report or None, stream or None))

    def reconstruct_decoded(self, indexed_shares: Sequence[Tuple[int, Sequence]], checks: Optional[int] = None, max_errors: int = 0,
                            correct: bool = False) -> Tuple[np.ndarray, "RevealDecode"]:
        """reconstruct_checked with the decoding finish: (values, RevealDecode)"""
        return self._reconstruct_with_checks(RevealDecode, indexed_shares, checks, max_errors, correct)

    # the erasure finish of a checked job: positions known to be unreliable (a refused sealed row) cost one check each, not two
    def finish_erasures_dev(self, d_ok: int, d_out: int, out_cap: int, d_report: int, max_errors: int = 0, correct: bool = False,
                            stream: int = 0) -> None:
        """ends a job begun by begin_checked_dev around the erased positions: d_ok is n_rows device words, 0 = erased (what
        update_sealed_rows_dev writes; 0: none), read by the kernels alone.  d_report: 16 + n_rows device words in
        finish_decoded_dev's layout, [6] = the number of erased positions, [7] = 1 when there are more than checks.  Nothing
        synchronises or reaches the host"""
        check(self._lib.sda_secret_reconstructor_finish_erasures_dev(self._h, d_ok or None, max_errors,
                                                                     capi.CHECK_CORRECT if correct else capi.CHECK_REPORT, d_out or None, out_cap,
                                                                     d_report or None, stream or None))

    def reconstruct_erasures(self, indexed_shares: Sequence[Tuple[int, Sequence]], erased: Optional[Sequence] = None,
                             checks: Optional[int] = None, max_errors: int = 0,
                             correct: bool = False) -> Tuple[np.ndarray, "RevealDecode", int, bool]:
        """reconstruct_decoded around the rows that `erased` flags (one truth value per row; None: none): (values, RevealDecode, the
        number of erased rows as the device counted them, whether they were more than checks)"""
        arrs, ptrs, lens = _rows([v for _, v in indexed_shares])
        cidx = _index_array([i for i, _ in indexed_shares])
        if checks is None and not isinstance(self.scheme, Additive):
            checks = self.default_checks(len(arrs))
        if erased is not None and len(erased) != len(arrs):
            raise SdaError(capi.ERR_INVALID_ARGUMENT, f"{len(erased)} erasure flags for {len(arrs)} rows")
        flags = None if erased is None else bytes(1 if e else 0 for e in erased)
        out = np.empty(max(self.dimension, 1), dtype=np.int64)
        report = (C.c_uint64 * (RevealDecode.HEAD + len(arrs)))()
        n_out = C.c_size_t()
        check(self._lib.sda_secret_reconstructor_reconstruct_erasures(
            self._h, cidx, ptrs, lens, len(arrs), max(int(checks or 0), 0), flags, max_errors,
            capi.CHECK_CORRECT if correct else capi.CHECK_REPORT, _ptr(out), self.dimension, C.byref(n_out), report))
        words = list(report)
        return out[:n_out.value].copy(), RevealDecode.from_words(words), int(words[6]), bool(words[7])

    def reconstruct_sealed_job_decoded(self, blob, indices: Sequence[int], pk: bytes, sk: bytes, checks: Optional[int] = None,
                                       max_errors: int = 0, correct: bool = False) -> Tuple[np.ndarray, "RevealDecode"]:
        """reconstruct_sealed_job_checked with the decoding finish: (values, RevealDecode).  A bad box still fails the reveal
        (sodium.rs:78-80)"""
        return self._reconstruct_sealed_job_with_checks(RevealDecode, "reconstruct_sealed_job_decoded", blob, indices, pk, sk, checks, max_errors, correct)

    def reconstruct_sealed_job(self, blob, indices: Optional[Sequence[int]], pk: bytes, sk: bytes,
                               row_len: Optional[int] = None) -> np.ndarray:
        """receive.rs:120-146 for an SDAJOBv1 blob of sealed clerking results, row i from clerk indices[i]: open every one,
        reconstruct.  One bad box fails the reveal ("Sodium decryption failure"), so does a payload that does not hold
        row_len values (default: ceil(dimension / k); Additive: the dimension)."""
        from .device import DeviceBuffer
        job = _parse_sealed_job("reconstruct_sealed_job", blob)
        row_len, n_out = self._sealed_job_shape(row_len)
        d_out = DeviceBuffer(max(n_out, 1))
        d_status = DeviceBuffer(1).zero()
        held = self._feed_sealed_job(job, indices, row_len, pk, sk, d_status.ptr)
        self.finish_dev(d_out.ptr, n_out)
        _raise_sealed_status(int(d_status.to_numpy()[0]))
        del held
        return d_out.to_numpy()[:n_out].copy()

    def _sealed_job_shape(self, row_len: Optional[int]) -> Tuple[int, int]:
        """(values per sealed clerking result, output length) of a job on this handle; row_len None: the scheme's own"""
        additive = isinstance(self.scheme, Additive)
        if row_len is None:
            row_len = self.dimension if additive else -(-self.dimension // self.scheme.secret_count)
        return row_len, (row_len if additive else self.dimension)

    def _feed_sealed_job(self, job: "JobContainer", indices: Optional[Sequence[int]], row_len: int, pk: bytes, sk: bytes,
                         d_status: int, checks: Optional[int] = None, d_ok: int = 0):
        """begin_dev (checks given: begin_checked_dev) + update_sealed_rows_dev over a parsed SDAJOBv1 SEALED job, row i from
        clerk indices[i]; the failures of the boxes land in *d_status and, with d_ok, one word per row in d_ok[].  Returns what
        must stay alive until the job's stream work is done"""
        from .device import DeviceBytes
        L = job.layout
        if checks is None:
            self.begin_dev(None if isinstance(self.scheme, Additive) else indices, L.rows, row_len)
        else:
            self.begin_checked_dev(indices, L.rows, row_len, checks)
        if not L.rows:
            return None
        d_job = DeviceBytes.from_bytes(job.blob)
        codec, box = VarintCodec(), SealedBox()
        self.update_sealed_rows_dev(codec, box, pk, sk, 0, d_job.ptr + L.payload_offset, L.slot_bytes,
                                    d_job.ptr + L.lengths_offset, L.rows, L.slot_bytes, d_status, d_ok)
        return d_job, codec, box


# ---- masking -------------------------------------------------------------------------------------------------
class SecretMasker(_Handle):
    """masking/mod.rs:13-15; impl none.rs:13-19, full.rs:21-35, chacha.rs:24-54."""
    _free = "sda_secret_masker_free"
    _value_mode = "sda_secret_masker_set_value_mode"

    def __init__(self, scheme: LinearMaskingScheme):
        super().__init__()
        self.scheme = scheme
        cs = scheme._c()
        check(self._lib.sda_secret_masker_new(C.byref(cs), C.byref(self._h)))

    def set_drbg_key(self, key: bytes):
        """TEST / BENCH ONLY: deterministic mode"""
        if len(key) != 32:
            raise ValueError("the CSPRNG key is exactly 32 bytes")
        check(self._lib.sda_secret_masker_set_drbg_key(self._h, (C.c_uint8 * 32)(*key)))

    def set_drbg_master_key(self, key: bytes):
        if len(key) != 32:
            raise ValueError("the CSPRNG key is exactly 32 bytes")
        check(self._lib.sda_secret_masker_set_drbg_master_key(self._h, (C.c_uint8 * 32)(*key)))

    def set_drbg_rounds(self, rounds: int):
        check(self._lib.sda_secret_masker_set_drbg_rounds(self._h, rounds))

    def mask(self, secrets, rand=None) -> Tuple[np.ndarray, np.ndarray]:
        s = _vec(secrets)
        cap = int(self._lib.sda_secret_masker_mask_len(self._h, s.size))
        mask = np.empty(max(cap, 1), dtype=np.int64)
        masked = np.empty(max(s.size, 1), dtype=np.int64)
        n_mask = C.c_size_t()
        if rand is None:
            rp, rl = None, 0
        else:
            r = _vec(rand)
            rp, rl = _ptr(r), r.size
        _check_mask(self._lib.sda_secret_masker_mask(self._h, _ptr(s), s.size, rp, rl, _ptr(mask), cap,
                                                     C.byref(n_mask), _ptr(masked)))
        return mask[:n_mask.value].copy(), masked[:s.size].copy()

    def mask_batch_dev(self, d_secrets: int, participants: int, length: int, secrets_stride: int, d_masks: int,
                       mask_stride: int, d_masked: int, masked_stride: int, first_participant: int = 0,
                       stream: int = 0) -> None:
        """participate.rs:52-54 for a device-resident tile (Full / None schemes)"""
        check(self._lib.sda_secret_masker_mask_batch_dev(self._h, d_secrets, participants, length, secrets_stride,
                                                         first_participant, d_masks or None, mask_stride, d_masked,
                                                         masked_stride, stream or None))

    def mask_sealed_rows_dev(self, codec: "VarintCodec", box: "SealedBox", recipient_pk: bytes, d_secrets: int, participants: int,
                             length: int, secrets_stride: int, d_masked: int, masked_stride: int, d_boxes: int, slot_bytes: int,
                             d_row_bytes: int, first_participant: int = 0, esk: Optional[bytes] = None, stream: int = 0) -> None:
        """participate.rs:52-72 for a device-resident tile: the masked secrets to d_masked, participant p's mask sealed to the
        recipient into d_boxes + p * slot_bytes, d_row_bytes[p] = payload + 48 (0: refused - check it before using d_masked).
        Full: no mask and no plaintext varint reaches device memory.  ChaCha: the sealed mask is the participant's seed.
        None has no recipient encryption (SDA_ERR_UNSUPPORTED: mask_batch_dev).  esk injects participants*32 bytes (tests only)."""
        assert len(recipient_pk) == 32 and (esk is None or len(esk) == 32 * participants)
        check(self._lib.sda_secret_masker_mask_sealed_rows_dev(
            self._h, codec._h, box._h, recipient_pk, esk, d_secrets or None, participants, length, secrets_stride, first_participant,
            d_masked or None, masked_stride, d_boxes, slot_bytes, d_row_bytes, stream or None))


class MaskCombiner(_Handle):
    """masking/mod.rs:21-23; impl none.rs:21-26, full.rs:37-52, chacha.rs:56-77."""
    _free = "sda_mask_combiner_free"
    _value_mode = "sda_mask_combiner_set_value_mode"

    def __init__(self, scheme: LinearMaskingScheme):
        super().__init__()
        self.scheme = scheme
        cs = scheme._c()
        check(self._lib.sda_mask_combiner_new(C.byref(cs), C.byref(self._h)))

    def combine(self, masks: Sequence) -> np.ndarray:
        arrs, ptrs, lens = _rows(masks)
        if isinstance(self.scheme, ChaCha):
            cap = self.scheme.dimension
        else:
            cap = arrs[0].size if arrs else 0
        out = np.empty(max(cap, 1), dtype=np.int64)
        n_out = C.c_size_t()
        _check_mask(self._lib.sda_mask_combiner_combine(self._h, ptrs, lens, len(arrs), _ptr(out), cap, C.byref(n_out)))
        return out[:n_out.value].copy()

    # streaming device form (receive.rs:101-118 with the masks in HBM): no update synchronises or copies to the host
    def begin_dev(self, dimension: int, stream: int = 0) -> None:
        check(self._lib.sda_mask_combiner_begin_dev(self._h, dimension, stream or None))
        self._dimension = dimension

    def update_dev(self, d_rows: int, rows: int, row_len: int, row_stride: int, stream: int = 0) -> None:
        """rows of masks in HBM: ChaCha seeds (words used `as u32`, the first 8 count) or Full mask vectors"""
        _check_mask(self._lib.sda_mask_combiner_update_dev(self._h, d_rows or None, rows, row_len, row_stride, stream or None))

    def update_sealed_rows_dev(self, codec: "VarintCodec", box: "SealedBox", pk: bytes, sk: bytes, d_boxes: int,
                               slot_bytes: int, d_row_bytes: int, rows: int, max_box_bytes: int, d_status: int, d_ok: int = 0,
                               stream: int = 0) -> None:
        """the participants' mask encryptions while they are still sealed boxes (the SDAJOBv1 SEALED layout).
        *d_status & 16: some box failed, the result must not be used (sodium.rs:78-80)"""
        check(self._lib.sda_mask_combiner_update_sealed_rows_dev(self._h, codec._h if codec else None, box._h if box else None,
                                                                 pk, sk, d_boxes, slot_bytes, d_row_bytes, rows, max_box_bytes,
                                                                 d_ok or None, d_status, stream or None))

    def finish_dev(self, d_out: int, out_cap: int, stream: int = 0) -> None:
        check(self._lib.sda_mask_combiner_finish_dev(self._h, d_out or None, out_cap, stream or None))

    def combine_sealed_job(self, blob, pk: bytes, sk: bytes, dimension: Optional[int] = None) -> np.ndarray:
        """receive.rs:101-118 for an SDAJOBv1 blob of sealed mask encryptions: open every one, combine the masks.  One bad
        box fails the job ("Sodium decryption failure"), so does a payload that is no varint vector.  ChaCha: the result
        has the scheme's dimension (chacha.rs:58); Full: `dimension` is the length every mask must have ("Wrong dimension"
        otherwise)."""
        from .device import DeviceBuffer
        job = _parse_sealed_job("combine_sealed_job", blob)
        dimension = self._sealed_job_dimension(dimension)
        d_out = DeviceBuffer(max(dimension, 1))
        d_status = DeviceBuffer(1).zero()
        held = self._feed_sealed_job(job, dimension, pk, sk, d_status.ptr)
        self.finish_dev(d_out.ptr, dimension)
        _raise_sealed_status(int(d_status.to_numpy()[0]))
        del held
        return d_out.to_numpy()[:dimension].copy()

    def _sealed_job_dimension(self, dimension: Optional[int]) -> int:
        if isinstance(self.scheme, ChaCha):
            return self.scheme.dimension
        if dimension is None:
            raise ValueError("combine_sealed_job needs the masks' dimension for this scheme")
        return dimension

    def _feed_sealed_job(self, job: "JobContainer", dimension: int, pk: bytes, sk: bytes, d_status: int):
        """begin_dev + update_sealed_rows_dev over a parsed SDAJOBv1 SEALED job of mask encryptions; the failures of the boxes
        land in *d_status.  Returns what must stay alive until the job's stream work is done"""
        from .device import DeviceBytes
        L = job.layout
        self.begin_dev(dimension)
        if not L.rows:
            return None
        d_job = DeviceBytes.from_bytes(job.blob)
        codec, box = VarintCodec(), SealedBox()
        self.update_sealed_rows_dev(codec, box, pk, sk, d_job.ptr + L.payload_offset, L.slot_bytes,
                                    d_job.ptr + L.lengths_offset, L.rows, L.slot_bytes, d_status)
        return d_job, codec, box


class SecretUnmasker(_Handle):
    """masking/mod.rs:29-31; impl none.rs:28-33, full.rs:54-67, chacha.rs:79-93."""
    _free = "sda_secret_unmasker_free"
    _value_mode = "sda_secret_unmasker_set_value_mode"

    def __init__(self, scheme: LinearMaskingScheme):
        super().__init__()
        self.scheme = scheme
        cs = scheme._c()
        check(self._lib.sda_secret_unmasker_new(C.byref(cs), C.byref(self._h)))

    def unmask(self, values: Tuple[Sequence, Sequence]) -> np.ndarray:
        mask, masked = _vec(values[0]), _vec(values[1])
        out = np.empty(max(masked.size, 1), dtype=np.int64)
        _check_mask(self._lib.sda_secret_unmasker_unmask(self._h, _ptr(mask), mask.size, _ptr(masked), masked.size,
                                                         _ptr(out)))
        return out[:masked.size].copy()

    def unmask_dev(self, d_mask: int, d_masked: int, length: int, d_out: int, stream: int = 0) -> None:
        check(self._lib.sda_secret_unmasker_unmask_dev(self._h, d_mask or None, d_masked, length, d_out, stream or None))

    def unmask_jobs_dev(self, combiner: Optional["MaskCombiner"], reconstructor: "SecretReconstructor", d_out: int, out_cap: int,
                        d_status_masks: int = 0, d_status_results: int = 0, stream: int = 0) -> None:
        """the recipient's last step (receive.rs:148-156) from the two device jobs' sums: what reconstructor.finish_dev,
        combiner.finish_dev and unmask_dev give, in one kernel, with neither the combined mask nor the masked output in HBM.
        Ends both jobs.  d_status_*: the status words of the jobs' sealed updates as gates - one of them non-zero when the
        kernel runs and nothing is stored to d_out.  combiner None: a None unmasker only"""
        _check_mask(self._lib.sda_secret_unmasker_unmask_jobs_dev(
            self._h, combiner._h if combiner is not None else None, reconstructor._h if reconstructor is not None else None,
            d_status_masks or None, d_status_results or None, d_out or None, out_cap, stream or None))

    def unmask_checked_jobs_dev(self, combiner: Optional["MaskCombiner"], reconstructor: "SecretReconstructor", end: int, d_out: int,
                                out_cap: int, d_report: int, d_ok: int = 0, max_errors: int = 0, correct: bool = False,
                                d_status_masks: int = 0, d_status_results: int = 0, results_pass_bits: int = 0, stream: int = 0) -> None:
        """unmask_jobs_dev for a CHECKED reconstructor job: end (capi.CHECKED_END_LOCATE / _DECODE / _ERASURES) names the finish -
        finish_checked_dev, finish_decoded_dev, finish_erasures_dev - whose verdicts and report (d_report, that finish's words) are
        wanted; d_out is that finish's output unmasked, from one kernel, with neither the masked output nor the combined mask in
        HBM.  Ends both jobs.  d_ok: the erasure end's flags; max_errors as for the named finish.  The gate: *d_status_masks != 0
        or (*d_status_results & ~results_pass_bits) != 0 when the kernel runs and nothing is stored to d_out - the report is
        written all the same; results_pass_bits is 0, or 16 for the caller who repairs refused boxes"""
        _check_mask(self._lib.sda_secret_unmasker_unmask_checked_jobs_dev(
            self._h, combiner._h if combiner is not None else None, reconstructor._h if reconstructor is not None else None, end,
            d_ok or None, max_errors, capi.CHECK_CORRECT if correct else capi.CHECK_REPORT, d_status_masks or None,
            d_status_results or None, results_pass_bits, d_out or None, out_cap, d_report or None, stream or None))


# ---- factory (client/src/crypto/mod.rs:58-66) ---------------------------------------------------------------
class CryptoModule:
    """The reference's factory object; the keystore plays no part on this path."""

    def new_share_generator(self, scheme): return ShareGenerator(scheme)
    def new_share_combiner(self, scheme): return ShareCombiner(scheme)
    def new_secret_reconstructor(self, scheme, dimension): return SecretReconstructor(scheme, dimension)
    def new_secret_masker(self, scheme): return SecretMasker(scheme)
    def new_mask_combiner(self, scheme): return MaskCombiner(scheme)
    def new_secret_unmasker(self, scheme): return SecretUnmasker(scheme)


@dataclass
class RecipientOutput:
    """client/src/receive.rs:7-21."""
    modulus: int
    values: np.ndarray

    def positive(self) -> "RecipientOutput":
        v = _vec(self.values)
        out = np.empty(max(v.size, 1), dtype=np.int64)
        check(capi.load().sda_positive(_ptr(v), v.size, self.modulus, _ptr(out)))
        return RecipientOutput(self.modulus, out[:v.size].copy())


@dataclass
class Aggregation:
    """The compute-relevant fields of protocol/src/resources.rs:44-67."""
    vector_dimension: int
    modulus: int
    masking_scheme: LinearMaskingScheme
    committee_sharing_scheme: LinearSecretSharingScheme


def full_aggregation(aggregation: Aggregation, inputs: Sequence[Sequence[int]], mask_rand=None, share_rand=None,
                     clerk_subset: Optional[Sequence[int]] = None, value_mode=CANONICAL) -> dict:
    """The three callers' data flow - participate.rs:52-76, the snapshot transposition
    (server/src/stores.rs:86-101), clerk.rs:85-86, receive.rs:101-156 - with the HIP core in place of
    the reference's crypto module.  Returns every intermediate.  value_mode=RUST_SIGNED asks every handle for the
    reference's own signed representatives (packed Shamir's generator / reconstructor stay canonical: tss's values)."""
    crypto = CryptoModule()
    a = aggregation
    n = a.committee_sharing_scheme.output_size()
    masks, maskeds, shares = [], [], []
    signed_sharing = value_mode == RUST_SIGNED and isinstance(a.committee_sharing_scheme, Additive)
    masker = crypto.new_secret_masker(a.masking_scheme).set_value_mode(value_mode)
    generator = crypto.new_share_generator(a.committee_sharing_scheme)
    if signed_sharing:
        generator.set_value_mode(RUST_SIGNED)
    for p, secrets in enumerate(inputs):
        if len(secrets) != a.vector_dimension:
            raise ValueError("The input length does not match the aggregation.")      # participate.rs:44-46
        m, ms = masker.mask(secrets, None if mask_rand is None else mask_rand[p])      # participate.rs:53-54
        masks.append(m); maskeds.append(ms)
        shares.append(generator.generate(ms, None if share_rand is None else share_rand[p]))   # :75-76
    combiner = crypto.new_share_combiner(a.committee_sharing_scheme).set_value_mode(value_mode)
    clerk_sums = [combiner.combine([shares[p][c] for p in range(len(inputs))]) for c in range(n)]   # clerk.rs:85-86
    mask = (crypto.new_mask_combiner(a.masking_scheme).set_value_mode(value_mode).combine(masks)
            if a.masking_scheme.has_mask() else np.empty(0, dtype=np.int64))             # receive.rs:102-118
    subset = list(range(n)) if clerk_subset is None else list(clerk_subset)
    rec = crypto.new_secret_reconstructor(a.committee_sharing_scheme, a.vector_dimension)
    if signed_sharing:
        rec.set_value_mode(RUST_SIGNED)
    masked_output = rec.reconstruct([(c, clerk_sums[c]) for c in subset])                # receive.rs:140-144
    output = crypto.new_secret_unmasker(a.masking_scheme).set_value_mode(value_mode).unmask((mask, masked_output))  # receive.rs:149-152
    return {"masks": masks, "masked": maskeds, "shares": shares, "clerk_sums": clerk_sums,
            "combined_mask": mask, "masked_output": masked_output, "output": output,
            "positive": RecipientOutput(a.modulus, output).positive().values}


def participate_sealed(aggregation: Aggregation, secrets_2d, recipient_pk: bytes, clerk_pks: Sequence[bytes],
                       first_participant: int = 0, mask_esk: Optional[bytes] = None, share_esk: Optional[bytes] = None):
    """new_participation (participate.rs:37-113) for a tile of P participants, from the secrets to wire bytes in two device
    calls: SecretMasker.mask_sealed_rows_dev (masked secrets, which stay on the device, and the P sealed masks), then
    ShareGenerator.generate_sealed_rows_dev on the masked secrets.  Returns (mask_job, clerk_jobs): the SDAJOBv1 SEALED blob
    of the P mask boxes - the argument of MaskCombiner.combine_sealed_job; None for NoMask, whose secrets are shared as they
    are (participate.rs:56-57) - and the n blobs of P share boxes each, clerk c's being the argument of
    ShareCombiner.clerk_sealed_job.  A sharing shape generate_sealed_rows_dev refuses raises its error unchanged.
    mask_esk / share_esk inject P*32 / n*P*32 bytes of ephemeral secrets (tests only)."""
    from .device import DeviceBuffer, DeviceBytes
    a = aggregation
    m = np.ascontiguousarray(secrets_2d, dtype=np.int64)
    if m.ndim != 2:
        raise ValueError("participate_sealed takes a matrix: one participant's secrets per row")
    P, length = m.shape
    if length != a.vector_dimension:
        raise ValueError("The input length does not match the aggregation.")             # participate.rs:44-46
    n = a.committee_sharing_scheme.output_size()
    if len(clerk_pks) != n:
        raise ValueError(f"one key per clerk: {n} keys, got {len(clerk_pks)}")
    codec, box = VarintCodec(), SealedBox()
    d_secrets = DeviceBuffer.from_numpy(m) if m.size else None
    d_ptr = d_secrets.ptr if m.size else 0

    def jobs_of(d_boxes, d_lens, slot, groups):
        """`groups` SDAJOBv1 SEALED blobs of P rows each out of the slotted rows of a device call"""
        lens = np.frombuffer(d_lens.to_bytes(groups * P * 8), dtype="<u8")
        if (lens == 0).any():
            raise SdaError(capi.ERR_INVALID_ARGUMENT, "sealing refused: a public key is a small-order point (all-zero shared secret)")
        raw = d_boxes.to_bytes(groups * P * slot)
        return [bytes(JobContainer.build(capi.JOB_SEALED, [raw[r * slot:r * slot + int(lens[r])] for r in range(g * P, (g + 1) * P)]))
                for g in range(groups)]

    mask_job = None
    if a.masking_scheme.has_mask():
        masker = SecretMasker(a.masking_scheme)
        slot = codec.slot_size(int(masker._lib.sda_secret_masker_mask_len(masker._h, length))) + SealedBox.SEALBYTES
        d_boxes, d_lens = DeviceBytes(max(P * slot, 16)), DeviceBytes(max(P * 8, 8)).zero()
        d_masked = DeviceBuffer(max(m.size, 2))
        masker.mask_sealed_rows_dev(codec, box, recipient_pk, d_ptr, P, length, length, d_masked.ptr if m.size else 0, length,
                                    d_boxes.ptr, slot, d_lens.ptr, first_participant, mask_esk)
        mask_job = jobs_of(d_boxes, d_lens, slot, 1)[0] if P else bytes(JobContainer.build(capi.JOB_SEALED, []))
        d_ptr = d_masked.ptr if m.size else 0
    generator = ShareGenerator(a.committee_sharing_scheme)
    slot = codec.slot_size(generator.batch_count(length)) + SealedBox.SEALBYTES
    d_boxes, d_lens = DeviceBytes(max(n * P * slot, 16)), DeviceBytes(max(n * P * 8, 8)).zero()
    generator.generate_sealed_rows_dev(codec, box, clerk_pks, d_ptr, P, length, length, d_boxes.ptr, slot, d_lens.ptr,
                                       first_participant, share_esk)
    return mask_job, jobs_of(d_boxes, d_lens, slot, n)


def _parse_reveal_jobs(name: str, masking_scheme, mask_job, result_job, recipient_pk: bytes, recipient_sk: bytes):
    """the front of every reveal from wire bytes: the keys are 32 bytes, a mask job comes with a scheme that has masks and only
    then, both blobs parse -> (the mask job or None, the results' job)"""
    if len(recipient_pk) != 32 or len(recipient_sk) != 32:
        raise SdaError(capi.ERR_INVALID_ARGUMENT, "the recipient's keys are 32 bytes each")
    if masking_scheme.has_mask() != (mask_job is not None):
        raise SdaError(capi.ERR_INVALID_ARGUMENT, "a mask job goes with a masking scheme that has masks, None with NoMask")
    return _parse_sealed_job(name, mask_job) if mask_job is not None else None, _parse_sealed_job(name, result_job)


def _check_result_indices(indices: Optional[Sequence[int]], rows: int, optional: bool) -> None:
    """one clerk index per clerking result; optional (Additive): None is as good"""
    if (indices is None and not optional) or (indices is not None and len(indices) != rows):
        raise SdaError(capi.ERR_INVALID_ARGUMENT, f"{0 if indices is None else len(indices)} indices for {rows} clerking results")


def reveal_sealed(aggregation: Aggregation, mask_job, result_job, indices: Optional[Sequence[int]], recipient_pk: bytes,
                  recipient_sk: bytes) -> RecipientOutput:
    """reveal_aggregation (receive.rs:80-157) from wire bytes, the counterpart of participate_sealed and
    ShareCombiner.clerk_sealed_job: mask_job is the SDAJOBv1 SEALED blob of the participants' mask encryptions (None for
    NoMask), result_job the one of the clerking results, row i from clerk indices[i] (Additive: indices may be None).  Both jobs
    are fed from the sealed boxes, then SecretUnmasker.unmask_jobs_dev folds and unmasks their sums with both status words as
    gates; the words and the output come back in one copy.  One bad box fails the reveal ("Sodium decryption failure"), then
    "Wrong dimension", then a malformed varint stream, whichever of the two jobs it came from."""
    from .device import DeviceBuffer
    a = aggregation
    sch, msch = a.committee_sharing_scheme, a.masking_scheme
    masks, results = _parse_reveal_jobs("reveal_sealed", msch, mask_job, result_job, recipient_pk, recipient_sk)
    _check_result_indices(indices, results.layout.rows, optional=isinstance(sch, Additive))
    reconstructor = SecretReconstructor(sch, a.vector_dimension)
    row_len, n_out = reconstructor._sealed_job_shape(None)
    unmasker = SecretUnmasker(msch)
    combiner = MaskCombiner(msch) if masks is not None else None
    # [0]: the mask job's status word, [1]: the clerking results', [2 ..): the output, 16-byte aligned
    d_buf = DeviceBuffer(2 + max(n_out, 1)).zero()
    held = []
    if combiner is not None:                 # ChaCha: the scheme's dimension; one that is not n_out is the reference's assert_eq! (chacha.rs:83)
        held.append(combiner._feed_sealed_job(masks, combiner._sealed_job_dimension(n_out), recipient_pk, recipient_sk, d_buf.at(0)))
    held.append(reconstructor._feed_sealed_job(results, indices, row_len, recipient_pk, recipient_sk, d_buf.at(1)))
    unmasker.unmask_jobs_dev(combiner, reconstructor, d_buf.at(2), n_out, d_buf.at(0), d_buf.at(1))
    back = d_buf.to_numpy()
    del held
    _raise_sealed_status(int(back[0]) | int(back[1]))
    return RecipientOutput(a.modulus, back[2:2 + n_out].copy())


def reveal_sealed_checked(aggregation: Aggregation, mask_job, result_job, indices: Sequence[int], recipient_pk: bytes,
                          recipient_sk: bytes, checks: Optional[int] = None, correct: bool = False):
    """reveal_sealed for a packed sharing scheme with the clerking results checked against each other: the results' job carries
    `checks` parity columns (None: min(n_rows - (t + k), 4)), and the reveal ends in SecretUnmasker.unmask_checked_jobs_dev with
    finish_checked_dev's end - one kernel over both jobs' sums, both status words as its gates.
    Returns (RecipientOutput, RevealCheck); correct=True repairs every batch that one clerking result alone spoils.  The failures of
    reveal_sealed stay: a bad box fails the reveal whatever the check says (sodium.rs:78-80)."""
    return _reveal_sealed_with_checks(RevealCheck, "reveal_sealed_checked", aggregation, mask_job, result_job, indices, recipient_pk,
                                      recipient_sk, checks, 0, correct)


def reveal_sealed_decoded(aggregation: Aggregation, mask_job, result_job, indices: Sequence[int], recipient_pk: bytes,
                          recipient_sk: bytes, checks: Optional[int] = None, max_errors: int = 0, correct: bool = False):
    """reveal_sealed_checked with finish_decoded_dev's end: up to max_errors (0: floor(checks / 2))
    disagreeing clerking results per batch are named and, with correct=True, repaired.  Returns (RecipientOutput, RevealDecode).
    A bad box still fails the reveal (sodium.rs:78-80)."""
    return _reveal_sealed_with_checks(RevealDecode, "reveal_sealed_decoded", aggregation, mask_job, result_job, indices, recipient_pk,
                                      recipient_sk, checks, max_errors, correct)


class RevealRepair(NamedTuple):
    """what reveal_sealed_repaired returns: the output, the report, the status word of the clerking results' sealed update (bit 16:
    some box was refused) and the number of refused boxes as the device counted them; unrepaired: they were more than checks"""
    output: RecipientOutput
    decode: RevealDecode
    status: int
    refused: int
    unrepaired: bool


def reveal_sealed_repaired(aggregation: Aggregation, mask_job, result_job, indices: Sequence[int], recipient_pk: bytes,
                           recipient_sk: bytes, checks: Optional[int] = None, max_errors: int = 0, correct: bool = True) -> RevealRepair:
    """reveal_sealed_decoded that REPAIRS refused clerking results instead of failing on them - the deliberate alternative to the
    reference's rule (sodium.rs:78-80), for a caller who prefers the other clerks' answer to none.  The sealed update's d_ok words
    go to finish_erasures_dev's end of SecretUnmasker.unmask_checked_jobs_dev untouched and unread: a refused box is an erasure and
    costs one check, not two; bit 16 of the results' status word does not shut that call's gate.
    The status word of the clerking results is RETURNED, not raised, for its bit 16; every other failure - a bad mask box, a wrong
    dimension, a malformed stream - fails the reveal as in reveal_sealed."""
    output, report, status = _reveal_sealed_with_checks(RevealDecode, "reveal_sealed_repaired", aggregation, mask_job, result_job, indices,
                                                        recipient_pk, recipient_sk, checks, max_errors, correct, repair=True)
    return RevealRepair(output, RevealDecode.from_words(report), status, int(report[6]), bool(report[7]))


def _reveal_sealed_with_checks(kind, name: str, aggregation: Aggregation, mask_job, result_job, indices, recipient_pk: bytes,
                               recipient_sk: bytes, checks: Optional[int], max_errors: int, correct: bool, repair: bool = False):
    """reveal_sealed_checked (kind RevealCheck: finish_checked_dev's end, max_errors is not read), reveal_sealed_decoded
    (RevealDecode: finish_decoded_dev's end) and, with repair, reveal_sealed_repaired (finish_erasures_dev's end around the rows the
    sealed update refused; returns (output, report words, the results' status word) and leaves bit 16 of that word to the caller)"""
    from .device import DeviceBuffer
    a = aggregation
    sch, msch = a.committee_sharing_scheme, a.masking_scheme
    masks, results = _parse_reveal_jobs(name, msch, mask_job, result_job, recipient_pk, recipient_sk)
    if isinstance(sch, Additive):
        raise SdaError(capi.ERR_UNSUPPORTED, "additive sharing has no redundancy to check")
    rows = results.layout.rows
    _check_result_indices(indices, rows, optional=False)
    reconstructor = SecretReconstructor(sch, a.vector_dimension)
    row_len, n_out = reconstructor._sealed_job_shape(None)
    checks = reconstructor.default_checks(rows) if checks is None else checks
    unmasker = SecretUnmasker(msch)
    combiner = MaskCombiner(msch) if masks is not None else None
    # [0]: the mask job's status word, [1]: the clerking results', [2 .. 2 + words): the report, then the output and, with repair,
    # the rows' ok words (two 32-bit words per entry)
    cap = max(n_out, 1)
    words = kind.HEAD + rows
    first = 2 + words
    d_buf = DeviceBuffer(first + cap + ((rows + 1) // 2 if repair else 0)).zero()
    d_ok = d_buf.at(first + cap) if repair else 0
    end = capi.CHECKED_END_ERASURES if repair else capi.CHECKED_END_LOCATE if kind is RevealCheck else capi.CHECKED_END_DECODE
    held = []
    if combiner is not None:
        held.append(combiner._feed_sealed_job(masks, combiner._sealed_job_dimension(n_out), recipient_pk, recipient_sk, d_buf.at(0)))
    held.append(reconstructor._feed_sealed_job(results, indices, row_len, recipient_pk, recipient_sk, d_buf.at(1), checks=checks, d_ok=d_ok))
    unmasker.unmask_checked_jobs_dev(combiner, reconstructor, end, d_buf.at(first), n_out, d_buf.at(2), d_ok, max_errors, correct,
                                     d_buf.at(0), d_buf.at(1), 16 if repair else 0)
    back = d_buf.to_numpy()
    del held
    status = int(back[1]) & 0xFFFFFFFF
    _raise_sealed_status(int(back[0]) | (status & ~16 if repair else status))
    output = RecipientOutput(a.modulus, back[first:first + n_out].copy())
    report = back[2:first].view(np.uint64).tolist()
    return (output, report, status) if repair else (output, kind.from_words(report))


# ---- share-vector wire codec -------------------------------------------------------------
class VarintCodec(_Handle):
    """zig-zag LEB128 codec of share vectors: what `ShareEncryptor::encrypt` does before sealing
    (encryption/sodium.rs:36-41) and `ShareDecryptor::decrypt` after opening (:83-89)."""
    _free = "sda_varint_codec_free"

    def __init__(self):
        super().__init__()
        check(self._lib.sda_varint_codec_new(C.byref(self._h)))

    def encode(self, shares) -> bytes:
        v = _vec(shares)
        out = np.empty(max(v.size * 10, 1), dtype=np.uint8)
        n = C.c_size_t()
        check(self._lib.sda_varint_encode(self._h, _ptr(v), v.size, out.ctypes.data_as(capi.c_u8p), v.size * 10, C.byref(n)))
        return out[:n.value].tobytes()

    def decode(self, raw: bytes) -> np.ndarray:
        b = np.frombuffer(raw, dtype=np.uint8)
        out = np.empty(max(b.size, 1), dtype=np.int64)
        n = C.c_size_t()
        check(self._lib.sda_varint_decode(self._h, b.ctypes.data_as(capi.c_u8p), b.size, _ptr(out), b.size, C.byref(n)))
        return out[:n.value].copy()

    def encode_dev(self, d_values: int, rows: int, length: int, row_stride: int, d_out: int, out_cap: int,
                   d_row_offsets: int = 0, stream: int = 0) -> int:
        total = C.c_uint64()
        check(self._lib.sda_varint_encode_dev(self._h, d_values, rows, length, row_stride, d_out, out_cap,
                                              d_row_offsets or None, C.byref(total), stream or None))
        return total.value

    def slot_size(self, length: int) -> int:
        return self._lib.sda_varint_slot_size(length)

    def encode_rows_dev(self, d_values: int, rows: int, length: int, row_stride: int, d_out: int, slot_bytes: int,
                        d_row_bytes: int, stream: int = 0) -> None:
        """single pass: row r -> d_out + r*slot_bytes, its length -> d_row_bytes[r]"""
        check(self._lib.sda_varint_encode_rows_dev(self._h, d_values, rows, length, row_stride, d_out, slot_bytes,
                                                   d_row_bytes, stream or None))

    def decode_rows_dev(self, d_bytes: int, slot_bytes: int, d_row_bytes: int, rows: int, length: int, d_values: int,
                        row_stride: int, d_status: int, stream: int = 0) -> None:
        check(self._lib.sda_varint_decode_rows_dev(self._h, d_bytes, slot_bytes, d_row_bytes, rows, length, d_values,
                                                   row_stride, d_status, stream or None))

    def decode_dev(self, d_bytes: int, n_bytes: int, d_row_offsets: int, rows: int, length: int, d_values: int,
                   row_stride: int, d_status: int, stream: int = 0) -> None:
        check(self._lib.sda_varint_decode_dev(self._h, d_bytes, n_bytes, d_row_offsets or None, rows, length, d_values,
                                              row_stride, d_status, stream or None))


# ---- clerking-job container + base64 `Binary` payloads -------------------------------------
class JobContainer:
    """SDAJOBv1: a ClerkingJob's `encryptions: Vec<Encryption>` (protocol/src/resources.rs:128-139) as one binary blob
    with fixed slots, laid out so the device calls consume it in place (include/sda_hip.h).  Host-side byte layout."""

    def __init__(self, blob: bytearray, layout: "capi.JobLayout"):
        self.blob, self.layout = blob, layout

    @classmethod
    def build(cls, kind: int, payloads: Sequence[bytes], slot_bytes: Optional[int] = None) -> "JobContainer":
        lib = capi.load()
        rows = len(payloads)
        slot = lib.sda_job_slot_size(max((len(p) for p in payloads), default=0)) if slot_bytes is None else slot_bytes
        size = lib.sda_job_container_size(rows, slot)
        if rows and size == 0:
            raise ValueError("slot_bytes must be a multiple of 16")
        blob = bytearray(max(size, 64))
        buf = (C.c_uint8 * len(blob)).from_buffer(blob)
        lay = capi.JobLayout()
        check(lib.sda_job_container_init(buf, len(blob), kind, rows, slot, C.byref(lay)))
        for r, p in enumerate(payloads):
            check(lib.sda_job_container_set_row(buf, len(blob), r, bytes(p), len(p)))
        del buf
        return cls(blob, lay)

    @classmethod
    def parse(cls, blob: bytes) -> "JobContainer":
        b = bytearray(blob)
        lay = capi.JobLayout()
        check(capi.load().sda_job_container_parse((C.c_uint8 * len(b)).from_buffer(b), len(b), C.byref(lay)))
        return cls(b, lay)

    def rows(self) -> List[bytes]:
        L = self.layout
        lens = np.frombuffer(self.blob, dtype="<u8", count=L.rows, offset=L.lengths_offset)
        return [bytes(self.blob[L.payload_offset + r * L.slot_bytes:L.payload_offset + r * L.slot_bytes + int(lens[r])])
                for r in range(L.rows)]

    def __bytes__(self):
        return bytes(self.blob)


def base64_decode_rows_dev(d_text: int, text_slot: int, d_text_bytes: int, rows: int, max_chars: int, d_out: int,
                           out_slot: int, d_out_bytes: int, d_status: int, d_row_status: int = 0, d_text_offsets: int = 0,
                           stream: int = 0) -> None:
    """Binary::from_base64 (helpers.rs:182-184) for `rows` payloads resident in HBM"""
    check(capi.load().sda_base64_decode_rows_dev(d_text, d_text_offsets or None, text_slot, d_text_bytes, rows, max_chars,
                                                 d_out, out_slot, d_out_bytes, d_status, d_row_status or None,
                                                 stream or None))


def base64_encode_rows_dev(d_in: int, in_slot: int, d_in_bytes: int, rows: int, max_bytes: int, d_text: int,
                           text_slot: int, d_text_bytes: int, stream: int = 0) -> None:
    """Binary::to_base64 (helpers.rs:178-180) for `rows` payloads resident in HBM"""
    check(capi.load().sda_base64_encode_rows_dev(d_in, in_slot, d_in_bytes, rows, max_bytes, d_text, text_slot,
                                                 d_text_bytes, stream or None))


# ---- sealed boxes: encryption/sodium.rs:33-46 (encrypt), :72-92 (decrypt) ----------------------
class SealedBox(_Handle):
    """libsodium crypto_box_seal / crypto_box_seal_open on the GPU, one payload (host forms) or a whole job (rows)."""
    _free = "sda_sealedbox_free"
    SEALBYTES = 48

    def __init__(self):
        super().__init__()
        check(self._lib.sda_sealedbox_new(C.byref(self._h)))

    def public_key(self, sk: bytes) -> bytes:
        """X25519(sk, 9): the public half of a key pair (crypto_scalarmult_base) - for tests and tools"""
        assert len(sk) == 32
        out = C.create_string_buffer(32)
        check(self._lib.sda_sealedbox_public_key(self._h, sk, out))
        return out.raw

    def seal(self, message: bytes, pk: bytes, esk: Optional[bytes] = None) -> bytes:
        """sealedbox::seal (sodium.rs:43); esk injects the ephemeral secret key (tests only)"""
        assert len(pk) == 32 and (esk is None or len(esk) == 32)
        out = np.empty(len(message) + 48, dtype=np.uint8)
        check(self._lib.sda_sealedbox_seal(self._h, pk, esk, bytes(message), len(message), out.ctypes.data_as(C.c_void_p), out.size))
        return out.tobytes()

    def open(self, box: bytes, pk: bytes, sk: bytes) -> bytes:
        """sealedbox::open (sodium.rs:78); raises SdaError("Sodium decryption failure") like the reference's Err (:80)"""
        assert len(pk) == 32 and len(sk) == 32
        out = np.empty(max(len(box), 1), dtype=np.uint8)
        n = C.c_size_t()
        check(self._lib.sda_sealedbox_open(self._h, pk, sk, bytes(box), len(box), out.ctypes.data_as(C.c_void_p), out.size, C.byref(n)))
        return out[:n.value].tobytes()

    def open_rows_dev(self, pk: bytes, sk: bytes, d_boxes: int, slot_bytes: int, d_row_bytes: int, rows: int, max_box_bytes: int,
                      d_out: int, out_slot: int, d_out_bytes: int, d_status: int, d_ok: int = 0, stream: int = 0) -> None:
        check(self._lib.sda_sealedbox_open_rows_dev(self._h, pk, sk, d_boxes, slot_bytes, d_row_bytes, rows, max_box_bytes, d_out,
                                                    out_slot, d_out_bytes, d_ok or None, d_status, stream or None))

    def seal_rows_dev(self, pks: Sequence[bytes], rows_per_key: int, d_msgs: int, msg_slot: int, d_msg_bytes: int, rows: int,
                      max_msg_bytes: int, d_boxes: int, slot_bytes: int, d_row_bytes: int, esk: Optional[bytes] = None,
                      stream: int = 0) -> None:
        allpk = b"".join(pks)
        assert len(allpk) == 32 * len(pks) and (esk is None or len(esk) == 32 * rows)
        check(self._lib.sda_sealedbox_seal_rows_dev(self._h, allpk, len(pks), rows_per_key, esk, d_msgs, msg_slot, d_msg_bytes, rows,
                                                    max_msg_bytes, d_boxes, slot_bytes, d_row_bytes, stream or None))

    def seal_share_rows_dev(self, codec: "VarintCodec", pks: Sequence[bytes], rows_per_key: int, d_values: int, rows: int,
                            length: int, row_stride: int, d_boxes: int, slot_bytes: int, d_row_bytes: int,
                            esk: Optional[bytes] = None, stream: int = 0) -> None:
        """share rows [rows][length] -> sealed boxes in one call (participate.rs:82-101): varint encode and XSalsa20 in one
        pass, no wire buffer.  Box r at d_boxes + r*slot_bytes, d_row_bytes[r] = payload bytes + 48 (0: the row was refused)"""
        allpk = b"".join(pks)
        assert len(allpk) == 32 * len(pks) and (esk is None or len(esk) == 32 * rows)
        check(self._lib.sda_sealedbox_seal_share_rows_dev(self._h, codec._h, allpk, len(pks), rows_per_key, esk, d_values or None, rows,
                                                          length, row_stride, d_boxes, slot_bytes, d_row_bytes, stream or None))


class ShareEncryptor:
    """encryption/sodium.rs:33-46: zig-zag varint encode every share, then seal the bytes for the clerk's key."""

    def __init__(self, pk: bytes):
        self.pk, self._box, self._codec = pk, SealedBox(), VarintCodec()

    def encrypt(self, shares, esk: Optional[bytes] = None) -> bytes:
        return self._box.seal(self._codec.encode(shares), self.pk, esk)

    def encrypt_rows(self, shares_2d, esk: Optional[bytes] = None) -> List[bytes]:
        """`encrypt` for a batch of share vectors (one per row) through ONE call of sda_sealedbox_seal_share_rows_dev: the
        counterpart of ShareCombiner.combine_sealed_job.  esk injects rows*32 bytes of ephemeral secrets (tests only)."""
        from .device import DeviceBuffer, DeviceBytes
        m = np.ascontiguousarray(shares_2d, dtype=np.int64)
        if m.ndim != 2:
            raise ValueError("encrypt_rows takes a matrix: one share vector per row")
        rows, length = m.shape
        if rows == 0:
            return []
        d_values = DeviceBuffer.from_numpy(m) if length else None
        slot = self._codec.slot_size(length) + SealedBox.SEALBYTES
        d_boxes, d_lens = DeviceBytes(rows * slot), DeviceBytes(rows * 8).zero()
        self._box.seal_share_rows_dev(self._codec, [self.pk], rows, d_values.ptr if length else 0, rows, length, length,
                                      d_boxes.ptr, slot, d_lens.ptr, esk)
        lens = np.frombuffer(d_lens.to_bytes(), dtype="<u8")
        if (lens == 0).any():
            raise SdaError(capi.ERR_INVALID_ARGUMENT, "sealing refused: the recipient public key is a small-order point (all-zero shared secret)")
        raw = d_boxes.to_bytes()
        return [bytes(raw[r * slot:r * slot + int(lens[r])]) for r in range(rows)]


class ShareDecryptor:
    """encryption/sodium.rs:72-92: open the sealed box, decode varints until the reader is empty."""

    def __init__(self, pk: bytes, sk: bytes):
        self.pk, self.sk, self._box, self._codec = pk, sk, SealedBox(), VarintCodec()

    def decrypt(self, encryption: bytes) -> np.ndarray:
        return self._codec.decode(self._box.open(encryption, self.pk, self.sk))
