"""sda_secret_unmasker_unmask_checked_jobs_dev on the GPU: the recipient's last step on a CHECKED reconstructor job and a mask
combiner job in one call.  Every case of tests/unmask_checked_cases.py is bit-exact against its Python-integer model - output and
report, in sentinel-filled buffers - and against the three-call chain (finish_checked_dev / finish_decoded_dev / finish_erasures_dev,
sda_mask_combiner_finish_dev, sda_secret_unmasker_unmask_dev) run on twin jobs; then the shut gate, the refusal order with several
faults per call, the handles reused across ends, a stream of the caller's, dimension 0 and the loop on sealed bytes through the
three reveal_sealed_* functions.  tests/test_unmask_checked_reach.py proves on the CPU what the table contains.  The table's borrowed
cases feed the rows of the finish tables' wide and steered cases, in one plaintext update_dev call."""
import numpy as np
import pytest

import reconstruct_stream_cases as rc
import unmask_checked_cases as kc

pytestmark = pytest.mark.gpu
SENTINEL = kc.SENTINEL
BASE = "k3_62-decode-correct-d766-rows2"


# ---- handles and jobs -------------------------------------------------------------------------------------------------------------
def sharing_of(case):
    from sda_amd import crypto
    p, k, t, n, w2, w3 = rc.SCHEMES[case.scheme]
    return crypto.PackedShamir(k, n, t, p, w2, w3)


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

    def fed(self, case=None, stream=0, mask_dim=None, checked=True, rows=None):
        """both jobs begun and fed from plaintext rows, the d_ok words uploaded"""
        from sda_amd.device import DeviceBuffer, DeviceBytes
        case = case or self.case
        b = kc.build(case.name)
        pos, B = len(case.indices), b.rows.shape[1]                                          # a borrowed case's rows are its source's, whole
        assert B >= kc.batches(case)
        if checked:
            self.reconstructor.begin_checked_dev(case.indices, pos, B, case.checks, stream)
        else:
            self.reconstructor.begin_dev(case.indices, pos, B, stream)
        d_rows = DeviceBuffer.from_numpy(b.rows)
        self.keep.append(d_rows)
        self.reconstructor.update_dev(0, d_rows.ptr, pos if rows is None else rows, B, stream)
        if self.combiner is not None:
            self.combiner.begin_dev(case.dim if mask_dim is None else mask_dim, stream)
            if kc.has_mask(case) and b.mask_rows.shape[0]:
                d_masks = DeviceBuffer.from_numpy(b.mask_rows)
                self.keep.append(d_masks)
                n, width = b.mask_rows.shape
                self.combiner.update_dev(d_masks.ptr, n, width, width, stream)
        ok = kc.ok_words(case)
        self.d_ok = 0
        if ok is not None:
            d = DeviceBytes.from_bytes(ok.astype("<u4").tobytes())
            self.keep.append(d)
            self.d_ok = d.ptr
        return self


def gate_pointers(case):
    """(keep-alive, d_status_masks, d_status_results) holding what the case says"""
    from sda_amd.device import DeviceBytes
    d = DeviceBytes.from_bytes(kc.gate_words(case).tobytes())
    if case.gates == "null":
        return d, 0, 0
    if case.gates == "equal":
        return d, d.ptr, d.ptr
    return d, d.ptr, d.ptr + 4


def sentinel_buffers(case):
    from sda_amd.device import DeviceBuffer
    head = case.offset // 8
    d_buf = DeviceBuffer.from_numpy(np.full(head + case.dim + kc.TAIL, SENTINEL, dtype=np.int64))
    d_rep = DeviceBuffer.from_numpy(np.full(kc.report_words(case) + kc.TAIL, SENTINEL, dtype=np.int64))
    assert d_buf.ptr % 16 == 0
    return d_buf, d_buf.at(head), d_rep


def run_new(case, h=None, stream=0):
    """the jobs fed, the one call -> the whole sentinel-filled output buffer (int64) and report buffer (uint64)"""
    h = h or Handles(case).fed(case, stream)
    keep, g_masks, g_results = gate_pointers(case)
    d_buf, d_out, d_rep = sentinel_buffers(case)
    h.unmasker.unmask_checked_jobs_dev(h.combiner, h.reconstructor, case.end, d_out, case.dim, d_rep.ptr, h.d_ok, case.cap,
                                       case.policy == kc.CORRECT, g_masks, g_results, case.pass_bits, stream)
    return d_buf.to_numpy(), d_rep.to_numpy().view(np.uint64)


def finish_by_chain(case, h, d_masked, d_report):
    correct = case.policy == kc.CORRECT
    if case.end == kc.LOCATE:
        h.reconstructor.finish_checked_dev(d_masked, case.dim, d_report, correct)
    elif case.end == kc.DECODE:
        h.reconstructor.finish_decoded_dev(d_masked, case.dim, d_report, case.cap, correct)
    else:
        h.reconstructor.finish_erasures_dev(h.d_ok, d_masked, case.dim, d_report, case.cap, correct)


def run_chain(case, h=None):
    """the three calls with their two intermediate buffers, on twin jobs -> out[0 .. dim), the report words"""
    from sda_amd.device import DeviceBuffer
    h = h or Handles(case).fed(case)
    L = case.dim
    d_masked, d_mask, d_out, d_rep = DeviceBuffer(L + 1), DeviceBuffer(L + 1), DeviceBuffer(L + 1), DeviceBuffer(kc.report_words(case))
    finish_by_chain(case, h, d_masked.ptr, d_rep.ptr)
    if h.combiner is not None:
        h.combiner.finish_dev(d_mask.ptr if kc.has_mask(case) else 0, L if kc.has_mask(case) else 0)
    h.unmasker.unmask_dev(d_mask.ptr if kc.has_mask(case) else 0, d_masked.ptr, L, d_out.ptr)
    return d_out.to_numpy()[:L], d_rep.to_numpy().view(np.uint64)


def raw_call(lib, u, c, r, end, d_out, cap, d_report, d_ok=0, max_errors=0, policy=0, g_masks=0, g_results=0, pass_bits=0):
    """the C entry point itself -> its status"""
    return lib.sda_secret_unmasker_unmask_checked_jobs_dev(u._h if u is not None else None, c._h if c is not None else None,
                                                           r._h if r is not None else None, end, d_ok or None, max_errors, policy,
                                                           g_masks or None, g_results or None, pass_bits, d_out or None, cap,
                                                           d_report or None, None)


# ---- 1. every case: the model, the chain, the sentinels, the kernels' names ---------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in kc.CASES])
def test_case_equals_the_model_and_the_chain(gpu, name):
    case = kc.BY_NAME[name]
    got, rep = run_new(case)
    kernels = gpu.sda_debug_last_kernel()
    want, want_rep = kc.want(name)
    head, words = case.offset // 8, kc.report_words(case)
    body = got[head:head + case.dim]
    print(f"{name}: L {case.dim}, mismatches vs model: output {int((got != want).sum())} of {got.size} buffer words, "
          f"report {int((rep != want_rep).sum())} of {rep.size}; report head {[int(x) for x in rep[:8 if case.end else 4]]}")
    assert (got[:head] == SENTINEL).all(), "stored before d_out"
    assert (got[head + case.dim:] == SENTINEL).all(), "stored at or past d_out + L"
    assert (rep[words:] == np.uint64(SENTINEL)).all(), "stored past the report"
    assert np.array_equal(rep, want_rep), "the report differs from the finish's model"
    assert np.array_equal(got, want), "the output differs from the Python-integer model"
    assert kernels == kc.KERNELS[case.end]
    chain, chain_rep = run_chain(case)
    assert gpu.sda_debug_last_kernel() != kernels
    print(f"{name}: mismatches vs the chain: report {int((rep[:words] != chain_rep).sum())}")
    assert np.array_equal(rep[:words], chain_rep), "the report differs from the finish's own, word for word"
    if kc.gate_shut(case):
        assert (body == SENTINEL).all()
    else:
        print(f"{name}: mismatches vs the chain: output {int((body != chain).sum())}")
        assert np.array_equal(body, chain), "differs from finish_*_dev + finish_dev + unmask_dev"


# ---- 2. a shut gate: no output, the finish's report, both jobs ended ---------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in kc.CASES if kc.gate_shut(c)])
def test_a_shut_gate_ends_both_jobs(gpu, name):
    from sda_amd import capi, crypto
    case = kc.BY_NAME[name]
    h = Handles(case).fed(case)
    got, rep = run_new(case, h)
    assert (got == SENTINEL).all(), "a failed reveal stored an output"
    assert [int(x) for x in rep[:kc.report_words(case)]] == list(kc.model(name).report)
    d_buf, d_out, d_rep = sentinel_buffers(case)
    with pytest.raises(crypto.SdaError) as e:
        finish_by_chain(case, h, d_out, d_rep.ptr)
    assert e.value.code == capi.ERR_STATE
    if kc.has_mask(case):
        with pytest.raises(crypto.SdaError) as e:
            h.combiner.finish_dev(d_out, case.dim)
        assert e.value.code == capi.ERR_STATE
    # a begin_dev and a begin_checked_dev afterwards succeed, and the next reveal on the handles is right
    h.reconstructor.begin_dev(case.indices, len(case.indices), kc.batches(case))
    open_case = case._replace(gates="null", offset=0)
    h.fed(open_case)
    got, rep = run_new(open_case, h)
    chain, chain_rep = run_chain(case)
    assert np.array_equal(got[:case.dim], chain) and np.array_equal(rep[:kc.report_words(case)], chain_rep)


# ---- 3. the refusal order: several faults per call, the earlier one answers; both jobs stay usable ----------------------------------
def _refused(gpu, code, text, *args, **kw):
    assert raw_call(gpu, *args, **kw) == code, gpu.sda_last_error()
    assert text in gpu.sda_last_error().decode(), gpu.sda_last_error()


def test_the_refusal_order(gpu):
    from sda_amd import capi, crypto
    case = kc.BY_NAME[BASE]
    L = case.dim
    h = Handles(case).fed(case)
    u, c, r = h.unmasker, h.combiner, h.reconstructor
    d_buf, d_out, d_rep = sentinel_buffers(case)
    rep = d_rep.ptr
    bad, state = capi.ERR_INVALID_ARGUMENT, capi.ERR_STATE
    D = kc.DECODE
    # 1 before everything: NULL handles win over an unknown end, a bad policy and bad pass bits
    _refused(gpu, bad, "unmasker is NULL", None, c, None, 9, d_out, L, rep, policy=7, pass_bits=3)
    _refused(gpu, bad, "reconstructor is NULL", u, c, None, 9, d_out, L, rep, policy=7, pass_bits=3)
    _refused(gpu, bad, "mask combiner is NULL", u, None, r, 9, d_out, L, rep, pass_bits=3)
    other = crypto.MaskCombiner(crypto.Full(kc.Q61))
    _refused(gpu, bad, "different masking schemes", u, other, r, 9, 0, 0, 0)
    idle = crypto.SecretReconstructor(sharing_of(case), L)
    _refused(gpu, state, "unmask before the reconstructor's begin", u, c, idle, 9, 0, 0, 0, pass_bits=3)
    # 2 the end, before the finish's refusals (max_errors, policy, NULL buffers) and everything behind them
    _refused(gpu, bad, "end = 9", u, c, r, 9, 0, 0, 0, max_errors=9, policy=7, pass_bits=3)
    _refused(gpu, bad, "end = -1", u, c, r, -1, d_out, L, rep)
    # 3 the finish's own, in its order: max_errors, the policy, d_out, out_cap, d_report - each before the pass bits
    _refused(gpu, bad, "max_errors = 3", u, c, r, D, 0, 0, 0, max_errors=3, policy=7, pass_bits=3)
    _refused(gpu, bad, "max_errors = 3", u, c, r, kc.ERASURES, 0, 0, 0, max_errors=3, policy=7, pass_bits=3)
    _refused(gpu, bad, "policy", u, c, r, D, 0, 0, 0, policy=7, pass_bits=3)
    _refused(gpu, bad, "policy", u, c, r, kc.LOCATE, 0, 0, 0, max_errors=3, policy=7)          # LOCATE does not read max_errors
    _refused(gpu, bad, "d_out is NULL", u, c, r, D, 0, 0, 0, pass_bits=3)
    _refused(gpu, bad, "output buffer too small", u, c, r, D, d_out, L - 1, 0, pass_bits=3)
    _refused(gpu, bad, "d_report is NULL", u, c, r, D, d_out, L, 0, pass_bits=3)
    # 7 the pass bits, last
    for bits in (1, 3, 17, 32):
        _refused(gpu, bad, f"results_pass_bits = {bits}", u, c, r, D, d_out, L, rep, pass_bits=bits)
    # both jobs are as they were: the chain ends them and gives the case's values
    assert (d_buf.to_numpy() == SENTINEL).all() and (d_rep.to_numpy() == SENTINEL).all()
    chain, chain_rep = run_chain(case, h)
    want, want_rep = kc.want(BASE)
    head = case.offset // 8
    assert np.array_equal(chain, want[head:head + L]) and np.array_equal(chain_rep, want_rep[:kc.report_words(case)])


def test_the_refusals_of_the_jobs_states(gpu):
    from sda_amd import capi, crypto
    from sda_amd.device import DeviceBuffer
    case = kc.BY_NAME[BASE]
    L = case.dim
    d_buf, d_out, d_rep = sentinel_buffers(case)
    d_tmp = DeviceBuffer(L)                                                          # where the jobs ended on the way write
    rep = d_rep.ptr
    state = capi.ERR_STATE
    # 3 a plain job: SDA_ERR_STATE in finish_with_checks' words - before the mask job's state (4) and the mask dimension (6)
    h = Handles(case).fed(case, checked=False)
    h.combiner.finish_dev(d_tmp.ptr, L)                                                  # the mask job is over: fault 4 beside fault 3
    _refused(gpu, state, "begun with begin_dev", h.unmasker, h.combiner, h.reconstructor, kc.DECODE, d_out, L, rep, pass_bits=3)
    h.reconstructor.finish_dev(d_tmp.ptr, L)
    # 3 a position not fed, before 4
    h = Handles(case).fed(case, rows=len(case.indices) - 1)
    h.combiner.finish_dev(d_tmp.ptr, L)
    _refused(gpu, state, "positions were not fed", h.unmasker, h.combiner, h.reconstructor, kc.DECODE, d_out, L, rep, pass_bits=3)
    # 3 DECODE on a job with one check, with a bad policy beside it
    one = case._replace(checks=1)
    h = Handles(one).fed(one)
    _refused(gpu, capi.ERR_INVALID_ARGUMENT, "one check decodes nothing", h.unmasker, h.combiner, h.reconstructor, kc.DECODE, d_out, L, rep,
             policy=7)
    # 4 the mask job not begun, before the signed mode (5), the mask dimension (6) and the pass bits (7)
    h = Handles(case).fed(case)
    h.combiner.finish_dev(d_tmp.ptr, L)
    h.unmasker.set_value_mode("rust_signed")
    _refused(gpu, state, "unmask before the mask combiner's begin", h.unmasker, h.combiner, h.reconstructor, kc.DECODE, d_out, L, rep, pass_bits=3)
    # 5 the signed mode, before the mask dimension and the pass bits
    h.combiner.begin_dev(L - 1)
    _refused(gpu, capi.ERR_UNSUPPORTED, "SDA_VALUES_RUST_SIGNED", h.unmasker, h.combiner, h.reconstructor, kc.DECODE, d_out, L, rep, pass_bits=3)
    h.unmasker.set_value_mode("canonical")
    # 6 the mask dimension: the reference's assert_eq!, before the pass bits
    _refused(gpu, capi.ERR_ASSERTION, f"(mask {L - 1}, masked secrets {L})", h.unmasker, h.combiner, h.reconstructor, kc.DECODE, d_out, L, rep,
             pass_bits=3)
    with pytest.raises(AssertionError):
        h.unmasker.unmask_checked_jobs_dev(h.combiner, h.reconstructor, kc.DECODE, d_out, L, rep)
    assert (d_buf.to_numpy() == SENTINEL).all() and (d_rep.to_numpy() == SENTINEL).all()
    # the reconstructor's job survived all of it: end it by the finish and compare
    h.reconstructor.finish_decoded_dev(d_out, L, rep, case.cap, True)
    fin = kc.finish(BASE)
    assert np.array_equal(d_buf.to_numpy()[case.offset // 8:][:L], fin.out)
    assert [int(x) for x in d_rep.to_numpy().view(np.uint64)[:kc.report_words(case)]] == [int(w) for w in fin.report]


# ---- 4. the handles across ends, a stream of the caller's, dimension 0 ---------------------------------------------------------------
def test_one_set_of_handles_serves_every_end(gpu):
    """three reveals on ONE unmasker, combiner and reconstructor - locate, erasures, decode, then a plain job through unmask_jobs_dev"""
    base = kc.BY_NAME["k3_62-erasures-correct-d764-f1-e1"]
    h = Handles(base)
    for end, cap in ((kc.LOCATE, 0), (kc.ERASURES, 1), (kc.DECODE, 2), (kc.ERASURES, 0)):
        case = base._replace(end=end, cap=cap, gates="two")
        h.fed(case)
        got, rep = run_new(case, h)
        assert gpu.sda_debug_last_kernel() == kc.KERNELS[end]
        chain, chain_rep = run_chain(case)
        head, words = case.offset // 8, kc.report_words(case)
        print(f"end {kc.ENDS[end]}: report head {[int(x) for x in rep[:8 if end else 4]]}")
        assert np.array_equal(got[head:head + case.dim], chain) and np.array_equal(rep[:words], chain_rep)
        assert (rep[words:] == np.uint64(SENTINEL)).all() and (got[head + case.dim:] == SENTINEL).all()
    h.fed(base, checked=False)
    d_buf, d_out, d_rep = sentinel_buffers(base)
    h.unmasker.unmask_jobs_dev(h.combiner, h.reconstructor, d_out, base.dim)
    assert gpu.sda_debug_last_kernel() == b"unmask_finish_kernel"


def test_on_a_stream_of_the_callers(gpu):
    import ctypes as C
    from sda_amd import capi
    hooks = capi.hooks_library()
    stream = C.c_void_p()
    capi.check(hooks.sda_debug_stream_create(C.byref(stream)))
    try:
        for name in (BASE, "k3_62-erasures-correct-d764-f1-e1"):
            case = kc.BY_NAME[name]
            h = Handles(case).fed(case, stream.value)
            keep, g_masks, g_results = gate_pointers(case)
            d_buf, d_out, d_rep = sentinel_buffers(case)
            h.unmasker.unmask_checked_jobs_dev(h.combiner, h.reconstructor, case.end, d_out, case.dim, d_rep.ptr, h.d_ok, case.cap,
                                               case.policy == kc.CORRECT, g_masks, g_results, case.pass_bits, stream.value)
            capi.check(hooks.sda_debug_stream_synchronize(stream))
            want, want_rep = kc.want(name)
            assert np.array_equal(d_buf.to_numpy(), want) and np.array_equal(d_rep.to_numpy().view(np.uint64), want_rep)
    finally:
        capi.check(hooks.sda_debug_stream_destroy(stream))


@pytest.mark.parametrize("end", list(kc.ENDS))
def test_dimension_zero(gpu, end):
    """SDA_OK, the report initialised, nothing launched, both jobs ended"""
    from sda_amd import capi, crypto
    from sda_amd.device import DeviceBuffer
    base = kc.BY_NAME[BASE]
    rec = crypto.SecretReconstructor(sharing_of(base), 0)
    comb, unm = crypto.MaskCombiner(crypto.Full(kc.P62)), crypto.SecretUnmasker(crypto.Full(kc.P62))
    rec.begin_checked_dev(base.indices, 8, 0, 4)
    d_rows = DeviceBuffer(8)
    rec.update_dev(0, d_rows.ptr, 8, 0)
    comb.begin_dev(0)
    words = (4 if end == kc.LOCATE else 16) + 8
    d_rep = DeviceBuffer.from_numpy(np.full(words + 4, SENTINEL, dtype=np.int64))
    gpu.sda_debug_last_kernel()
    before = gpu.sda_debug_last_kernel()
    unm.unmask_checked_jobs_dev(comb, rec, end, 0, 0, d_rep.ptr)
    assert gpu.sda_debug_last_kernel() == before
    rep = [int(x) for x in d_rep.to_numpy().view(np.uint64)]
    none = (1 << 64) - 1
    assert rep[:words] == ([0, 0, 0, none] if end == kc.LOCATE else [0, 0, 0, none, none] + [0] * 11) + [0] * 8
    assert rep[words:] == [SENTINEL] * 4
    with pytest.raises(crypto.SdaError) as e:
        rec.finish_checked_dev(0, 0, d_rep.ptr)
    assert e.value.code == capi.ERR_STATE
    with pytest.raises(crypto.SdaError) as e:
        comb.finish_dev(0, 0)
    assert e.value.code == capi.ERR_STATE


# ---- 5. sealed end to end: participate_sealed -> clerk_sealed_job -> the three reveals ------------------------------------------------
@pytest.fixture(scope="module")
def sealed_loop(gpu):
    from sda_amd import crypto
    from test_reconstruct_stream_gpu import _keys
    p, k, t, n, w2, w3 = rc.SCHEMES["k3_62"]
    dim, P = 764, 3
    sharing = crypto.PackedShamir(k, n, t, p, w2, w3)
    agg = crypto.Aggregation(dim, p, crypto.Full(p), sharing)
    rng = np.random.default_rng(2101)
    secrets = rng.integers(0, p, size=(P, dim), dtype=np.int64)
    truth = (secrets.astype(object).sum(axis=0) % p).astype(np.int64)
    rpk, rsk = _keys(81)
    clerks = [_keys(90 + c) for c in range(n)]
    mask_job, clerk_jobs = crypto.participate_sealed(agg, secrets, rpk, [pk for pk, _ in clerks])
    comb = crypto.ShareCombiner(sharing)
    B = -(-dim // k)
    boxes = [bytes(comb.clerk_sealed_job(clerk_jobs[c], cpk, csk, rpk, B)) for c, (cpk, csk) in enumerate(clerks)]
    sums = [crypto.ShareDecryptor(rpk, rsk).decrypt(box) for box in boxes]
    return agg, mask_job, boxes, sums, truth, (rpk, rsk), B


def test_sealed_end_to_end(gpu, sealed_loop):
    from sda_amd import capi, crypto
    agg, mask_job, boxes, sums, truth, (rpk, rsk), B = sealed_loop
    p, n = agg.modulus, 8
    indices = list(range(n))
    enc = crypto.ShareEncryptor(rpk)
    clean_job = bytes(crypto.JobContainer.build(0, boxes))
    # clean results: every reveal gives the sum of the inputs and a clean report
    out, chk = crypto.reveal_sealed_checked(agg, mask_job, clean_job, indices, rpk, rsk)
    assert gpu.sda_debug_last_kernel() == kc.KERNELS[kc.LOCATE]
    assert np.array_equal(out.values, truth) and chk.clean and chk.blame == (0,) * n
    out, dec = crypto.reveal_sealed_decoded(agg, mask_job, clean_job, indices, rpk, rsk, correct=True)
    assert gpu.sda_debug_last_kernel() == kc.KERNELS[kc.DECODE]
    assert np.array_equal(out.values, truth) and dec.clean
    got = crypto.reveal_sealed_repaired(agg, mask_job, clean_job, indices, rpk, rsk)
    assert gpu.sda_debug_last_kernel() == kc.KERNELS[kc.ERASURES]
    assert np.array_equal(got.output.values, truth) and got.status == 0 and got.refused == 0 and not got.unrepaired and got.decode.clean
    # two clerks with a bug: located by none, decoded and repaired by the decoding reveal
    wrong = list(sums)
    for liar in (2, 6):
        wrong[liar] = ((wrong[liar].astype(object) + 12345 + liar) % p).astype(np.int64)
    wrong_job = bytes(crypto.JobContainer.build(0, [enc.encrypt(s) for s in wrong]))
    plain = crypto.reveal_sealed(agg, mask_job, wrong_job, indices, rpk, rsk)
    out, chk = crypto.reveal_sealed_checked(agg, mask_job, wrong_job, indices, rpk, rsk, correct=True)
    assert chk.bad == B and chk.located == 0 and np.array_equal(out.values, plain.values)
    out, dec = crypto.reveal_sealed_decoded(agg, mask_job, wrong_job, indices, rpk, rsk)
    assert np.array_equal(out.values, plain.values) and dec.decoded == B and dec.corrected == 0
    out, dec = crypto.reveal_sealed_decoded(agg, mask_job, wrong_job, indices, rpk, rsk, correct=True)
    assert np.array_equal(out.values, truth) and dec.corrected == B and dec.blame == tuple(B if i in (2, 6) else 0 for i in range(n))
    # a tampered box: the strict reveals fail (the gate was shut: sodium.rs:78-80), the repairing one repairs
    tampered = list(boxes)
    tampered[5] = tampered[5][:37] + bytes([tampered[5][37] ^ 0x40]) + tampered[5][38:]
    bad_job = bytes(crypto.JobContainer.build(0, tampered))
    for strict in (lambda: crypto.reveal_sealed_checked(agg, mask_job, bad_job, indices, rpk, rsk, correct=True),
                   lambda: crypto.reveal_sealed_decoded(agg, mask_job, bad_job, indices, rpk, rsk, correct=True)):
        with pytest.raises(crypto.SdaError) as e:
            strict()
        assert e.value.code == capi.ERR_SODIUM_DECRYPTION
    got = crypto.reveal_sealed_repaired(agg, mask_job, bad_job, indices, rpk, rsk)
    assert got.status & 16 and got.refused == 1 and not got.unrepaired and got.decode.bad == 0
    assert np.array_equal(got.output.values, truth)
    # a tampered MASK box fails the repairing reveal too
    blob = bytearray(mask_job)
    layout = crypto.JobContainer.parse(bytes(mask_job)).layout
    blob[layout.payload_offset + 40] ^= 1
    with pytest.raises(crypto.SdaError) as e:
        crypto.reveal_sealed_repaired(agg, bytes(blob), clean_job, indices, rpk, rsk)
    assert e.value.code == capi.ERR_SODIUM_DECRYPTION
