"""sda_secret_unmasker_unmask_jobs_dev on the GPU: unmask() fed by the recipient's two device jobs (receive.rs:148-156).  Every case
of tests/unmask_jobs_cases.py is bit-exact against its Python-integer model and against the three-call chain
(sda_secret_reconstructor_finish_dev, sda_mask_combiner_finish_dev, sda_secret_unmasker_unmask_dev) run on twin jobs, and leaves the
sentinel around d_out alone; then the gates on tampered sealed boxes, every refusal, the state after success, a stream of the
caller's, the loop on sealed bytes through reveal_sealed, and the footprint.  tests/test_unmask_jobs_reach.py proves on the CPU what
the table contains."""
import ctypes as C

import numpy as np
import pytest

import reconstruct_stream_cases as rc
import unmask_jobs_cases as uc
from conftest import load_golden, use_test_hooks

pytestmark = pytest.mark.gpu
SENTINEL = uc.SENTINEL
KERNEL = b"unmask_finish_kernel"
BASE = "k3_62-full-d1000-off0"


# ---- handles and jobs -------------------------------------------------------------------------------------------------------------
def sharing_of(case):
    from sda_amd import crypto
    p, k, t, n, w2, w3 = rc.SCHEMES[case.scheme]
    return crypto.Additive(n, p) if uc.additive(case) else crypto.PackedShamir(k, n, t, p, w2, w3)


def masking_of(case):
    from sda_amd import crypto
    if case.masking == "full":
        return crypto.Full(case.q_mask)
    if case.masking == "chacha":
        return crypto.ChaCha(case.q_mask, case.dim, 128)
    return crypto.NoMask()


class Handles:
    def __init__(self, case):
        from sda_amd import crypto
        self.case = case
        self.unmasker = crypto.SecretUnmasker(masking_of(case))
        self.combiner = None if case.masking == "none-null" else crypto.MaskCombiner(masking_of(case))
        self.reconstructor = crypto.SecretReconstructor(sharing_of(case), case.dim)
        self.keep = []

    def begin(self, stream=0, mask_dim=None):
        case = self.case
        self.reconstructor.begin_dev(None if uc.additive(case) else case.indices, len(case.indices), uc.batches(case), stream)
        if self.combiner is not None:
            self.combiner.begin_dev(case.dim if mask_dim is None else mask_dim, stream)

    def feed_results(self, stream=0, first=0, count=None):
        from sda_amd.device import DeviceBuffer
        b = uc.build(self.case.name)
        count = len(self.case.indices) - first if count is None else count
        d_rows = DeviceBuffer.from_numpy(b.rows)
        self.keep.append(d_rows)
        B = uc.batches(self.case)
        self.reconstructor.update_dev(first, d_rows.at(first * B), count, B, stream)

    def feed_masks(self, stream=0):
        from sda_amd.device import DeviceBuffer
        b = uc.build(self.case.name)
        if not uc.has_mask(self.case) or b.mask_rows.shape[0] == 0:
            return
        d_masks = DeviceBuffer.from_numpy(b.mask_rows)
        self.keep.append(d_masks)
        rows, width = b.mask_rows.shape
        self.combiner.update_dev(d_masks.ptr, rows, width, width, stream)

    def fed(self, stream=0):
        self.begin(stream)
        self.feed_masks(stream)
        self.feed_results(stream)
        return self


def gate_words(case):
    """(keep-alive, d_status_masks, d_status_results) as the case asks; a shut gate holds 16, the failed-box bit"""
    from sda_amd.device import DeviceBytes
    words = np.zeros(2, dtype="<u4")
    if case.gates in ("closed-masks", "closed-equal"):
        words[0] = 16
    if case.gates == "closed-results":
        words[1] = 16
    d = DeviceBytes.from_bytes(words.tobytes())
    if case.gates == "null":
        return d, 0, 0
    if case.gates in ("equal", "closed-equal"):
        return d, d.ptr, d.ptr
    return d, d.ptr, d.ptr + 4


def sentinel_buffer(case):
    from sda_amd.device import DeviceBuffer
    head = case.offset // 8
    d = DeviceBuffer.from_numpy(np.full(head + case.dim + uc.TAIL, SENTINEL, dtype=np.int64))
    assert d.ptr % 16 == 0
    return d, d.at(head)


def run_new(case, h=None, stream=0):
    """the jobs fed, the one call -> the whole sentinel-filled buffer"""
    h = h or Handles(case).fed(stream)
    keep, g_masks, g_results = gate_words(case)
    d_buf, d_out = sentinel_buffer(case)
    h.unmasker.unmask_jobs_dev(h.combiner, h.reconstructor, d_out, case.dim, g_masks, g_results, stream)
    return d_buf.to_numpy()


def run_chain(case):
    """the three calls with their two intermediate buffers on twin jobs -> out[0 .. dim)"""
    from sda_amd.device import DeviceBuffer
    h = Handles(case).fed()
    L = case.dim
    d_masked, d_mask, d_out = DeviceBuffer(L + 1), DeviceBuffer(L + 1), DeviceBuffer(L + 1)
    h.reconstructor.finish_dev(d_masked.ptr, L)
    if h.combiner is not None:
        h.combiner.finish_dev(d_mask.ptr if uc.has_mask(case) else 0, L if uc.has_mask(case) else 0)
    h.unmasker.unmask_dev(d_mask.ptr if uc.has_mask(case) else 0, d_masked.ptr, L, d_out.ptr)
    return d_out.to_numpy()[:L]


def raw_call(lib, u, c, r, d_out, cap, g_masks=0, g_results=0, stream=0):
    """the C entry point itself -> its status"""
    return lib.sda_secret_unmasker_unmask_jobs_dev(u._h if u is not None else None, c._h if c is not None else None,
                                                   r._h if r is not None else None, g_masks or None, g_results or None, d_out or None, cap,
                                                   stream or None)


# ---- 1. every case: the model, the chain, the sentinel, the kernel's name ------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in uc.CASES])
def test_case_equals_the_model_and_the_chain(gpu, name):
    case = uc.BY_NAME[name]
    got = run_new(case)
    want = uc.want(name)
    head = case.offset // 8
    body = got[head:head + case.dim]
    print(f"{name}: L {case.dim}, mismatches vs model {int((got != want).sum())} of {got.size} buffer words")
    assert (got[:head] == SENTINEL).all(), "stored before d_out"
    assert (got[head + case.dim:] == SENTINEL).all(), "stored at or past d_out + L"
    assert np.array_equal(got, want), "differs from the Python-integer model"
    assert gpu.sda_debug_last_kernel() == KERNEL
    if uc.gate_shut(case):
        assert (body == SENTINEL).all()
    else:
        chain = run_chain(case)
        print(f"{name}: mismatches vs the chain {int((body != chain).sum())}")
        assert np.array_equal(body, chain), "differs from finish_dev + finish_dev + unmask_dev"


# ---- 2. the gates on sealed boxes -------------------------------------------------------------------------------------------------
def _sealed_setup(tamper):
    """BASE with its clerking results (tamper == 'results') or its masks (tamper == 'masks') fed as sealed boxes, one byte of one box
    flipped; the other job from plaintext rows.  -> (handles, status word of the masks, of the results, keep-alive)"""
    from sda_amd import crypto
    from sda_amd.device import DeviceBytes
    from test_reconstruct_stream_gpu import _host_boxes, _keys, upload_boxes
    case, b = uc.BY_NAME[BASE], uc.build(BASE)
    pk, sk = _keys(41)
    h = Handles(case)
    h.begin()
    codec, box = crypto.VarintCodec(), crypto.SealedBox()
    d_status = DeviceBytes(8).zero()
    rows = b.rows if tamper == "results" else b.mask_rows
    _, boxes = _host_boxes(rows, pk, 41)
    boxes[1] = boxes[1][:60] + bytes([boxes[1][60] ^ 0x04]) + boxes[1][61:]
    job = upload_boxes(boxes)
    if tamper == "results":
        h.feed_masks()
        h.reconstructor.update_sealed_rows_dev(codec, box, pk, sk, 0, job.d_boxes.ptr, job.slot, job.d_lens.ptr, job.rows, job.slot, d_status.ptr + 4)
    else:
        h.feed_results()
        h.combiner.update_sealed_rows_dev(codec, box, pk, sk, job.d_boxes.ptr, job.slot, job.d_lens.ptr, job.rows, job.slot, d_status.ptr)
    return h, d_status, (job, codec, box)


def _status(d_status):
    return [int(x) for x in np.frombuffer(d_status.to_bytes(), dtype="<u4")[:2]]


@pytest.mark.parametrize("tamper", ["results", "masks"])
def test_one_tampered_byte_shuts_the_gate(gpu, tamper):
    case = uc.BY_NAME[BASE]
    h, d_status, keep = _sealed_setup(tamper)
    d_buf, d_out = sentinel_buffer(case)
    h.unmasker.unmask_jobs_dev(h.combiner, h.reconstructor, d_out, case.dim, d_status.ptr, d_status.ptr + 4)
    got, st = d_buf.to_numpy(), _status(d_status)
    print(f"tampered {tamper}: status words {st}, words written {int((got != SENTINEL).sum())}")
    assert st == ([0, 16] if tamper == "results" else [16, 0])
    assert (got == SENTINEL).all(), "a failed reveal stored an output"
    assert gpu.sda_debug_last_kernel() == KERNEL
    # the jobs were ended all the same
    from sda_amd import capi, crypto
    with pytest.raises(crypto.SdaError) as e:
        h.reconstructor.finish_dev(d_out, case.dim)
    assert e.value.code == capi.ERR_STATE


@pytest.mark.parametrize("tamper", ["results", "masks"])
def test_without_gates_the_output_is_written(gpu, tamper):
    case = uc.BY_NAME[BASE]
    h, d_status, keep = _sealed_setup(tamper)
    d_buf, d_out = sentinel_buffer(case)
    h.unmasker.unmask_jobs_dev(h.combiner, h.reconstructor, d_out, case.dim)
    got = d_buf.to_numpy()
    assert 16 in _status(d_status)
    assert (got[:case.dim] != SENTINEL).all() and (got[:case.dim] < case.q_mask).all() and (got[:case.dim] >= 0).all()
    assert (got[case.dim:] == SENTINEL).all()


@pytest.mark.parametrize("tamper", ["results", "masks", None])
def test_equal_gate_pointers(gpu, tamper):
    """both jobs report into ONE status word, given as both gates"""
    from sda_amd import crypto
    from sda_amd.device import DeviceBytes
    from test_reconstruct_stream_gpu import _host_boxes, _keys, upload_boxes
    case, b = uc.BY_NAME[BASE], uc.build(BASE)
    pk, sk = _keys(43)
    h = Handles(case)
    h.begin()
    codec, box = crypto.VarintCodec(), crypto.SealedBox()
    d_status = DeviceBytes(4).zero()
    _, rboxes = _host_boxes(b.rows, pk, 43)
    _, mboxes = _host_boxes(b.mask_rows, pk, 44)
    if tamper == "results":
        rboxes[7] = rboxes[7][:33] + bytes([rboxes[7][33] ^ 0x80]) + rboxes[7][34:]
    if tamper == "masks":
        mboxes[0] = mboxes[0][:-1] + bytes([mboxes[0][-1] ^ 0x01])
    rjob, mjob = upload_boxes(rboxes), upload_boxes(mboxes)
    h.combiner.update_sealed_rows_dev(codec, box, pk, sk, mjob.d_boxes.ptr, mjob.slot, mjob.d_lens.ptr, mjob.rows, mjob.slot, d_status.ptr)
    h.reconstructor.update_sealed_rows_dev(codec, box, pk, sk, 0, rjob.d_boxes.ptr, rjob.slot, rjob.d_lens.ptr, rjob.rows, rjob.slot, d_status.ptr)
    d_buf, d_out = sentinel_buffer(case)
    h.unmasker.unmask_jobs_dev(h.combiner, h.reconstructor, d_out, case.dim, d_status.ptr, d_status.ptr)
    got = d_buf.to_numpy()
    status = int(np.frombuffer(d_status.to_bytes(), dtype="<u4")[0])
    if tamper is None:
        assert status == 0 and np.array_equal(got, uc.want(BASE))
    else:
        assert status == 16 and (got == SENTINEL).all()


# ---- 3. refusals: before any launch, both jobs left as they were ---------------------------------------------------------------------
def test_argument_refusals_leave_both_jobs_alive(gpu):
    from sda_amd import capi, crypto
    from sda_amd.device import DeviceBuffer
    case = uc.BY_NAME[BASE]
    L = case.dim
    h = Handles(case).fed()
    u, c, r = h.unmasker, h.combiner, h.reconstructor
    d_buf, d_out = sentinel_buffer(case)
    bad = capi.ERR_INVALID_ARGUMENT
    assert raw_call(gpu, None, c, r, d_out, L) == bad                                   # NULL u
    assert raw_call(gpu, u, c, None, d_out, L) == bad                                   # NULL r
    assert raw_call(gpu, u, None, r, d_out, L) == bad                                   # NULL c, a kind with masks
    assert raw_call(gpu, u, c, r, 0, L) == bad                                          # NULL d_out, L > 0
    assert raw_call(gpu, u, c, r, d_out, L - 1) == bad                                  # out_cap < L
    others = [crypto.Full(uc.Q61), crypto.ChaCha(uc.P62, L, 128), crypto.NoMask()]      # modulus, kind, None
    for scheme in others:
        assert raw_call(gpu, crypto.SecretUnmasker(scheme), c, r, d_out, L) == bad, scheme
        assert b"different masking schemes" in gpu.sda_last_error()
    for scheme in (crypto.Full(uc.Q61), crypto.NoMask()):                               # the same from the combiner's side, its job begun
        other = crypto.MaskCombiner(scheme)
        other.begin_dev(L)
        assert raw_call(gpu, u, other, r, d_out, L) == bad, scheme
    cu, cc = crypto.SecretUnmasker(crypto.ChaCha(uc.P62, L, 128)), crypto.MaskCombiner(crypto.ChaCha(uc.P62, L + 1, 128))
    cc.begin_dev(L + 1)
    assert raw_call(gpu, cu, cc, r, d_out, L) == bad                                    # ChaCha: the dimensions differ
    if gpu.sda_device_count() >= 2:                                                     # the three handles not on one device
        capi.check(gpu.sda_set_device(1))
        try:
            far_u, far_c = crypto.SecretUnmasker(masking_of(case)), crypto.MaskCombiner(masking_of(case))
            far_c.begin_dev(L)
        finally:
            capi.check(gpu.sda_set_device(0))
        assert raw_call(gpu, far_u, c, r, d_out, L) == bad
        assert raw_call(gpu, u, far_c, r, d_out, L) == bad
    u.set_value_mode("rust_signed")                                                     # SDA_VALUES_RUST_SIGNED on the unmasker
    assert raw_call(gpu, u, c, r, d_out, L) == capi.ERR_UNSUPPORTED
    u.set_value_mode("canonical")
    assert (d_buf.to_numpy() == SENTINEL).all(), "a refused call stored something"
    # none of them touched the jobs: the call now succeeds and gives the right output
    assert raw_call(gpu, u, c, r, d_out, L) == capi.OK
    assert np.array_equal(d_buf.to_numpy(), uc.want(BASE))


def test_state_refusals_leave_the_other_job_alive(gpu):
    from sda_amd import capi
    case = uc.BY_NAME[BASE]
    L, pos = case.dim, len(case.indices)
    # the reconstructor's job not begun
    h = Handles(case)
    h.combiner.begin_dev(L)
    h.feed_masks()
    d_buf, d_out = sentinel_buffer(case)
    assert raw_call(gpu, h.unmasker, h.combiner, h.reconstructor, d_out, L) == capi.ERR_STATE
    h.reconstructor.begin_dev(case.indices, pos, uc.batches(case))
    # ... begun, one position unfed: the text of finish_dev
    h.feed_results(first=0, count=pos - 1)
    assert raw_call(gpu, h.unmasker, h.combiner, h.reconstructor, d_out, L) == capi.ERR_STATE
    assert b"1 of the job's 8 positions were not fed" in gpu.sda_last_error()
    h.feed_results(first=pos - 1, count=1)
    assert (d_buf.to_numpy() == SENTINEL).all()
    assert raw_call(gpu, h.unmasker, h.combiner, h.reconstructor, d_out, L) == capi.OK      # the mask job and the fed rows survived
    assert np.array_equal(d_buf.to_numpy(), uc.want(BASE))
    # the mask combiner's job not begun
    h = Handles(case)
    h.reconstructor.begin_dev(case.indices, pos, uc.batches(case))
    h.feed_results()
    d_buf, d_out = sentinel_buffer(case)
    assert raw_call(gpu, h.unmasker, h.combiner, h.reconstructor, d_out, L) == capi.ERR_STATE
    h.combiner.begin_dev(L)
    h.feed_masks()
    assert (d_buf.to_numpy() == SENTINEL).all()
    assert raw_call(gpu, h.unmasker, h.combiner, h.reconstructor, d_out, L) == capi.OK
    assert np.array_equal(d_buf.to_numpy(), uc.want(BASE))


def _chain_halves(h, case):
    """both jobs ended by their own finish_dev -> (masked, mask): the proof that a refused call left them alive"""
    from sda_amd.device import DeviceBuffer
    L = case.dim
    mask_len = h.combiner._dimension
    d_masked, d_mask = DeviceBuffer(L + 1), DeviceBuffer(mask_len + 1)
    h.reconstructor.finish_dev(d_masked.ptr, L)
    h.combiner.finish_dev(d_mask.ptr, mask_len)
    return d_masked.to_numpy()[:L], d_mask.to_numpy()[:mask_len]


def test_a_mask_job_of_another_dimension_is_the_reference_assertion(gpu):
    """full.rs:58: assert_eq!(mask.len(), masked.len())"""
    from sda_amd import capi, crypto
    from sda_amd.device import DeviceBuffer
    case, b = uc.BY_NAME[BASE], uc.build(BASE)
    L = case.dim
    h = Handles(case)
    h.begin(mask_dim=L - 1)
    h.feed_results()
    d_masks = DeviceBuffer.from_numpy(np.ascontiguousarray(b.mask_rows[:, :L - 1]))
    h.combiner.update_dev(d_masks.ptr, 3, L - 1, L - 1)
    d_buf, d_out = sentinel_buffer(case)
    assert raw_call(gpu, h.unmasker, h.combiner, h.reconstructor, d_out, L) == capi.ERR_ASSERTION
    assert b"full.rs" in gpu.sda_last_error() or b"left == right" in gpu.sda_last_error()
    with pytest.raises(AssertionError):                                                 # the mirror: a panic of the reference
        h.unmasker.unmask_jobs_dev(h.combiner, h.reconstructor, d_out, L)
    assert (d_buf.to_numpy() == SENTINEL).all()
    m = uc.model(BASE)
    masked, mask = _chain_halves(h, case)
    assert list(map(int, masked)) == list(m.masked) and list(map(int, mask)) == list(m.mask[:L - 1])


def test_rust_signed_jobs_take_the_chain(gpu):
    """the value mode read into either job at its begin_dev: SDA_ERR_UNSUPPORTED, and the chain still serves both jobs"""
    from sda_amd import capi
    case = uc.BY_NAME["additive-full-d1000"]
    L = case.dim
    for who in ("reconstructor", "combiner"):
        h = Handles(case)
        getattr(h, who).set_value_mode("rust_signed")
        h.fed()
        getattr(h, who).set_value_mode("canonical")                                     # too late: the job read the mode when it began
        d_buf, d_out = sentinel_buffer(case)
        assert raw_call(gpu, h.unmasker, h.combiner, h.reconstructor, d_out, L) == capi.ERR_UNSUPPORTED, who
        assert (d_buf.to_numpy() == SENTINEL).all()
        m = uc.model(case.name)
        masked, mask = _chain_halves(h, case)
        q = case.q_mask                                                                 # the signed representatives of the same residues
        assert [int(x) % q for x in masked] == list(m.masked) and [int(x) % q for x in mask] == list(m.mask), who


def test_an_empty_job_launches_nothing_and_ends_both_jobs(gpu):
    from sda_amd import capi, crypto
    p = rc.SCHEMES["additive"][0]
    u, c, r = crypto.SecretUnmasker(crypto.Full(p)), crypto.MaskCombiner(crypto.Full(p)), crypto.SecretReconstructor(crypto.Additive(3, p), 0)
    r.begin_dev(None, 3, 0)
    r.update_dev(0, 0, 3, 0)
    c.begin_dev(0)
    before = gpu.sda_debug_last_kernel()
    assert raw_call(gpu, u, c, r, 0, 0) == capi.OK
    assert gpu.sda_debug_last_kernel() == before
    for finish in (lambda: r.finish_dev(0, 0), lambda: c.finish_dev(0, 0)):
        with pytest.raises(crypto.SdaError) as e:
            finish()
        assert e.value.code == capi.ERR_STATE


# ---- 4. after success -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [BASE, "k3_62-chacha-d1000", "k3_62-none-combiner-d1000"])
def test_success_ends_both_jobs_and_the_handles_begin_again(gpu, name):
    from sda_amd import capi, crypto
    from sda_amd.device import DeviceBuffer
    case = uc.BY_NAME[name]
    L = case.dim
    h = Handles(case).fed()
    assert np.array_equal(run_new(case, h), uc.want(name))
    d_scratch = DeviceBuffer(L + 1)
    for finish in (lambda: h.reconstructor.finish_dev(d_scratch.ptr, L), lambda: h.combiner.finish_dev(d_scratch.ptr, L)):
        with pytest.raises(crypto.SdaError) as e:
            finish()
        assert e.value.code == capi.ERR_STATE
    d_buf, d_out = sentinel_buffer(case)
    if uc.has_mask(case):                                                               # a second call finds no job either
        assert raw_call(gpu, h.unmasker, h.combiner, h.reconstructor, d_out, L) == capi.ERR_STATE
    h.fed()
    assert np.array_equal(run_new(case, h), uc.want(name))


# ---- 5. a stream of the caller's ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [BASE, "k3_62-chacha-rejecting-d8", "additive-crafted-d1000"])
def test_the_whole_job_on_a_stream_of_the_callers(gpu, name):
    from sda_amd import capi
    hooks = capi.hooks_library()
    stream = C.c_void_p()
    capi.check(hooks.sda_debug_stream_create(C.byref(stream)))
    try:
        case = uc.BY_NAME[name]
        h = Handles(case).fed(stream.value)
        keep, g_masks, g_results = gate_words(case)
        d_buf, d_out = sentinel_buffer(case)
        h.unmasker.unmask_jobs_dev(h.combiner, h.reconstructor, d_out, case.dim, g_masks, g_results, stream.value)
        capi.check(hooks.sda_debug_stream_synchronize(stream))
        assert np.array_equal(d_buf.to_numpy(), uc.want(name))
    finally:
        capi.check(hooks.sda_debug_stream_destroy(stream))


# ---- 6. the loop on sealed bytes ----------------------------------------------------------------------------------------------------
def _sealed_loop(agg, inputs, subset=None):
    """participate_sealed -> clerk_sealed_job per clerk -> reveal_sealed"""
    from oracle import sealedbox_oracle as so
    from sda_amd import capi, crypto
    sch, dim = agg.committee_sharing_scheme, agg.vector_dimension
    n = sch.output_size()
    rng = np.random.default_rng(n + dim)
    sks = [bytes(rng.integers(0, 256, 32, dtype=np.uint8)) for _ in range(n + 1)]
    pks = [so.x25519_base(s) for s in sks]
    rpk, rsk = pks[n], sks[n]
    mask_job, clerk_jobs = crypto.participate_sealed(agg, inputs, rpk, pks[:n])
    row_len = dim if isinstance(sch, crypto.Additive) else -(-dim // sch.secret_count)
    results = [crypto.ShareCombiner(sch).clerk_sealed_job(clerk_jobs[c], pks[c], sks[c], rpk, row_len) for c in range(n)]
    subset = list(range(n)) if subset is None else subset
    job = bytes(crypto.JobContainer.build(capi.JOB_SEALED, [results[c] for c in subset]))
    out = crypto.reveal_sealed(agg, mask_job, job, subset, rpk, rsk)
    assert out.modulus == agg.modulus
    return out, (mask_job, job, subset, rpk, rsk)


@pytest.mark.parametrize("kind", ["full-additive", "full-packed", "chacha-packed", "nomask"])
def test_the_loop_on_sealed_bytes(gpu, kind):
    import generate_sealed_cases as gs
    from sda_amd import capi, crypto
    case = gs.BY_NAME["additive-n3" if kind == "full-additive" else "B129"]
    q, dim = case["p"], case["len"]
    if case["additive"]:
        sch, subset = crypto.Additive(case["n"], q), None
    else:
        sch, subset = crypto.PackedShamir(case["k"], case["n"], case["t"], q, *gs.omegas(case)), [7, 0, 3, 5, 2]
    msch = crypto.ChaCha(q, dim, 128) if kind.startswith("chacha") else crypto.NoMask() if kind == "nomask" else crypto.Full(q)
    inputs = np.random.default_rng(24 + dim).integers(0, q, size=(24, dim), dtype=np.int64)
    agg = crypto.Aggregation(dim, q, msch, sch)
    out, (mask_job, job, subset, rpk, rsk) = _sealed_loop(agg, inputs, subset)
    assert gpu.sda_debug_last_kernel() == KERNEL
    truth = [sum(int(x) for x in inputs[:, i]) % q for i in range(dim)]
    assert list(map(int, out.values)) == truth
    # one tampered byte, in either job: the reference's error, mask job first
    L = crypto.JobContainer.parse(job).layout
    bad = bytearray(job)
    bad[L.payload_offset + L.slot_bytes + 50] ^= 1
    with pytest.raises(crypto.SdaError) as e:
        crypto.reveal_sealed(agg, mask_job, bytes(bad), subset, rpk, rsk)
    assert e.value.code == capi.ERR_SODIUM_DECRYPTION and e.value.message == "Sodium decryption failure"
    if mask_job is not None:
        M = crypto.JobContainer.parse(mask_job).layout
        bad = bytearray(mask_job)
        bad[M.payload_offset + 3 * M.slot_bytes + 40] ^= 0x20
        with pytest.raises(crypto.SdaError) as e:
            crypto.reveal_sealed(agg, bytes(bad), job, subset, rpk, rsk)
        assert e.value.code == capi.ERR_SODIUM_DECRYPTION
    # a clerking result of another length: "Wrong dimension"
    if not case["additive"]:
        short = crypto.Aggregation(dim + 3 * sch.secret_count, q, crypto.NoMask(), sch)
        with pytest.raises(crypto.SdaError) as e:
            crypto.reveal_sealed(short, None, job, subset, rpk, rsk)
        assert e.value.code == capi.ERR_WRONG_DIMENSION and e.value.message == "Wrong dimension"


@pytest.mark.parametrize("name", ["F2_with_fullmask", "F3_with_chachamask", "F4c_packedshamir_fullmask"])
def test_the_loop_on_sealed_bytes_gives_the_golden_outputs(gpu, name):
    from sda_amd import crypto
    from test_parity_gpu import _mask_scheme, _scheme
    sc = {s["name"]: s for s in load_golden("full_loop.json")["scenarios"]}[name]
    a = sc["aggregation"]
    agg = crypto.Aggregation(a["vector_dimension"], a["modulus"], _mask_scheme(a["masking_scheme"]), _scheme(a["committee_sharing_scheme"]))
    out, _ = _sealed_loop(agg, np.array(sc["inputs"], dtype=np.int64), sc["clerk_subset"])
    assert list(map(int, out.values)) == sc["stages"]["canonical"]["output"]
    assert list(map(int, out.positive().values)) == sc["expected_positive"]


# ---- 7. footprint -----------------------------------------------------------------------------------------------------------------
def test_footprint_no_intermediate_buffers(gpu):
    """Additive over 3 clerks, a Full mask of 32 participants, 200,000 values: the chain holds a combined-mask buffer and a
    masked-output buffer of 8 L = 1.6 MB each between its calls; the new call allocates nothing, so the allocator sees nothing newly
    held after it"""
    from sda_amd import capi, crypto
    from sda_amd.device import DeviceBuffer, synchronize
    lib = use_test_hooks()                                       # sda_debug_mem_info lives in the library with the test hooks
    P, L, q = 32, 200_000, rc.P62
    rng = np.random.default_rng(17)
    masks = rng.integers(0, q, size=(P, L), dtype=np.int64)
    rows = rng.integers(0, q, size=(3, L), dtype=np.int64)
    d_masks, d_rows, d_out = DeviceBuffer.from_numpy(masks), DeviceBuffer.from_numpy(rows), DeviceBuffer(L)
    want = ((rows.astype(object).sum(axis=0) % q - masks.astype(object).sum(axis=0) % q) % q).astype(np.int64)

    def free_now():
        synchronize()
        f, t = C.c_size_t(), C.c_size_t()
        capi.check(lib.sda_debug_mem_info(C.byref(f), C.byref(t)))
        return f.value

    def jobs():
        u, c, r = crypto.SecretUnmasker(crypto.Full(q)), crypto.MaskCombiner(crypto.Full(q)), crypto.SecretReconstructor(crypto.Additive(3, q), L)
        r.begin_dev(None, 3, L)
        r.update_dev(0, d_rows.ptr, 3, L)
        c.begin_dev(L)
        c.update_dev(d_masks.ptr, P, L, L)
        return u, c, r

    u, c, r = jobs()
    before = free_now()
    u.unmask_jobs_dev(c, r, d_out.ptr, L)
    grown = before - free_now()
    assert np.array_equal(d_out.to_numpy(), want)
    u2, c2, r2 = jobs()
    mid = free_now()
    d_masked, d_mask = DeviceBuffer(L), DeviceBuffer(L)
    r2.finish_dev(d_masked.ptr, L)
    c2.finish_dev(d_mask.ptr, L)
    u2.unmask_dev(d_mask.ptr, d_masked.ptr, L, d_out.ptr)
    chain = mid - free_now()
    print(f"two buffers of 8 L = {2 * 8 * L} B; newly held by the new call {grown} B, by the chain {chain} B")
    assert np.array_equal(d_out.to_numpy(), want)
    assert chain >= 2 * 8 * L
    assert grown == 0
