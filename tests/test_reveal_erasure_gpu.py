"""The erasure finish of the checked reveal on the GPU: sda_secret_reconstructor_finish_erasures_dev / reconstruct_erasures and
crypto.reveal_sealed_repaired.  Every case of tests/reveal_erasure_cases.py is fed by update_dev, its flags uploaded, and ended
under both policies; output, every report word and the sentinels past both buffers are bit-exact against the Python-integer model
(proven to be the definition by tests/test_reveal_erasure_reach.py).  Then: without erasures the call is finish_decoded_dev on a
twin job; what an erased row added does not matter; the refusals and their order; the host form; and sealed clerking results with
one and with f = c tampered boxes, whose d_ok words reach the finish untouched - and, on the 300-row committee, boxes 63 and 256
refused in two update calls.  No test provokes a fault: a refused box is an
ordinary status."""
import numpy as np
import pytest

import reveal_check_cases as vc
import reveal_decode_cases as dc
import reveal_erasure_cases as ec
from test_reveal_check_gpu import Feeder, _keys, _raises, run_unchecked, scheme_of, u32, upload_boxes
from test_reveal_decode_gpu import finish_decoded

pytestmark = pytest.mark.gpu
SENTINEL = 0x5A5A5A5A5A5A5A5A
KERNELS = b"reveal_erasure_setup_kernel + reveal_erasure_finish_kernel"


def finish_erasures(rec, case, ok, correct, max_errors=None):
    """finish_erasures_dev into sentinel-framed buffers: the report buffer starts as garbage (the call initialises it itself); ok:
    the flags as uint32 words (None: NULL), framed as well"""
    from sda_amd import capi
    from sda_amd.device import DeviceBuffer, DeviceBytes
    pos = len(case.indices)
    d_out = DeviceBuffer.from_numpy(np.full(case.dim + 8, SENTINEL, dtype=np.int64))
    d_report = DeviceBuffer.from_numpy(np.full(ec.HEAD + pos + 4, SENTINEL, dtype=np.int64))
    d_ok = None if ok is None else DeviceBytes.from_bytes(np.ascontiguousarray(ok, dtype="<u4").tobytes())
    rec.finish_erasures_dev(0 if d_ok is None else d_ok.ptr, d_out.ptr, case.dim, d_report.ptr, case.cap if max_errors is None else max_errors,
                            correct)
    assert capi.load().sda_debug_last_kernel() == KERNELS
    got, rep = d_out.to_numpy(), d_report.to_numpy()
    assert (got[case.dim:] == SENTINEL).all(), "finish_erasures_dev wrote past its output"
    assert (rep[ec.HEAD + pos:] == SENTINEL).all(), "finish_erasures_dev wrote past its report"
    if d_ok is not None:
        assert np.array_equal(u32(d_ok, pos), np.asarray(ok, dtype=np.uint32)), "finish_erasures_dev wrote to d_ok"
    return got[:case.dim], [int(x) for x in rep[:ec.HEAD + pos].view(np.uint64)]


def run_erasures(case, rows, correct, rec=None, ok="case"):
    from sda_amd import crypto
    from sda_amd.device import DeviceBuffer
    rec = rec or crypto.SecretReconstructor(scheme_of(case), case.dim)
    d_rows = DeviceBuffer.from_numpy(np.ascontiguousarray(rows))
    rec.begin_checked_dev(case.indices, rows.shape[0], rows.shape[1], case.checks)
    rec.update_dev(0, d_rows.ptr, rows.shape[0], rows.shape[1])
    return finish_erasures(rec, case, ec.ok_words(case) if isinstance(ok, str) else ok, correct)


# ---- 1. every case, both policies ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in ec.CASES])
def test_case_equals_the_model(gpu, name):
    from sda_amd import crypto
    case, b = ec.BY_NAME[name], ec.build(name)
    rec = crypto.SecretReconstructor(scheme_of(case), case.dim)
    plain_job = run_unchecked(case, b.rows)
    for correct in (False, True):
        want = ec.model_finish(case, b.rows, ec.CORRECT if correct else ec.REPORT)
        out, report = run_erasures(case, b.rows, correct, rec=rec)
        print(f"{name} {'correct' if correct else 'report'}: report {report[:ec.HEAD]} model {want.report[:ec.HEAD]}, "
              f"output mismatches {int((out != want.out).sum())}")
        assert report == want.report, correct
        assert np.array_equal(out, want.out), correct
        if not correct or len(case.erased) > case.checks:
            assert np.array_equal(out, plain_job), "the output differs from the unchecked job on the same rows"
    e = ec.cap_of(case)
    if len(case.erased) <= case.checks and len(set(b.faulty)) == 1 and len(b.faulty[0]) <= e:
        keep = [i for i in range(len(case.indices)) if i not in b.faulty[0] and i not in case.erased]
        others = crypto.SecretReconstructor(scheme_of(case), case.dim).reconstruct([(case.indices[i], b.rows[i]) for i in keep])
        assert np.array_equal(out, others), "SDA_CHECK_CORRECT differs from reconstruct() of the surviving rows"
        assert np.array_equal(out, b.want)


# ---- 2. no erasures: finish_decoded_dev on a twin job ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in ec.CASES if c.ok != "flags" and c.checks >= 2] +
                         ["k3_62-c4-d769-f0-e2-zero", "k3_62-c4-d769-f0-e1-zero"])
def test_without_erasures_it_is_the_decoding_finish(gpu, name):
    from sda_amd import crypto
    from sda_amd.device import DeviceBuffer
    case, b = ec.BY_NAME[name], ec.build(name)
    assert not case.erased
    twin = dc.Case(name, case.scheme, case.dim, case.indices, case.checks, case.cap, "sums", "none", "one", 0)
    d_rows = DeviceBuffer.from_numpy(np.ascontiguousarray(b.rows))
    for correct in (False, True):
        rec = crypto.SecretReconstructor(scheme_of(case), case.dim)
        rec.begin_checked_dev(case.indices, b.rows.shape[0], b.rows.shape[1], case.checks)
        rec.update_dev(0, d_rows.ptr, b.rows.shape[0], b.rows.shape[1])
        old_out, old_report = finish_decoded(rec, twin, correct)
        for ok in (None, np.full(len(case.indices), 0xFFFFFFFF, dtype=np.uint32), np.arange(1, len(case.indices) + 1, dtype=np.uint32)):
            out, report = run_erasures(case, b.rows, correct, ok=ok)
            assert report == old_report and np.array_equal(out, old_out), correct


# ---- 3. whatever an erased row added -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["k3_62-c4-d764-f2-e1-zero", "k3_62-c4-d764-f2-e1-spoiled", "k3_62-c1-d764-f1-e0-zero", "k8_62-c16-d805-f8-e4-random",
                                  "k3_wide-c16-d769-f5-e5-zero"])
def test_what_an_erased_row_added_does_not_matter(gpu, name):
    """a position refused (it added nothing) and the same position fed with random values: identical d_out and report"""
    case = ec.BY_NAME[name]
    first = run_erasures(case, ec.refilled(name, "zero"), True)
    second = run_erasures(case, ec.refilled(name, "random"), True)
    third = run_erasures(case, ec.build(name).rows, True)
    assert first[1] == second[1] == third[1]
    assert np.array_equal(first[0], second[0]) and np.array_equal(first[0], third[0])
    assert np.array_equal(first[0], ec.build(name).want)


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_are_the_decoding_finishs_and_leave_the_job_usable(gpu):
    """finish_erasures_dev refuses in finish_decoded_dev's order -  no job > plain job > unfed positions > max_errors > policy >
    d_out > out_cap > d_report  - with its texts and codes, and accepts a job of one check.  Calls that carry two faults at once say
    which comes first; every refused call leaves the job to finish with the model's output."""
    import ctypes as C
    from sda_amd import capi, crypto
    from sda_amd.device import DeviceBuffer
    case, b = ec.BY_NAME[ec.E2E], ec.build(ec.E2E)
    L, pos = b.row_len, len(case.indices)
    d_out, d_report = DeviceBuffer(case.dim + 1), DeviceBuffer(ec.HEAD + pos)
    d_rows = DeviceBuffer.from_numpy(np.ascontiguousarray(b.rows))
    rec = crypto.SecretReconstructor(scheme_of(case), case.dim)
    erasures = lambda policy, out, cap, report, max_errors=0: gpu.sda_secret_reconstructor_finish_erasures_dev(
        rec._h, None, max_errors, policy, out, cap, report, None)
    decoded = lambda policy, out, cap, report, max_errors=0: gpu.sda_secret_reconstructor_finish_decoded_dev(
        rec._h, max_errors, policy, out, cap, report, None)

    def same_refusal(args, code, word, **kw):
        texts = []
        for fin in (decoded, erasures):
            status = fin(*args, **kw)
            texts.append(gpu.sda_last_error().decode())
            assert status == code and word in texts[-1], (status, texts[-1], code, word)
        assert texts[0] == texts[1], texts

    BAD_POLICY = 7
    same_refusal((capi.CHECK_CORRECT, None, 0, None), capi.ERR_STATE, "before begin")                       # no job + NULL buffers
    rec.begin_dev(case.indices, pos, L)                                                                    # a plain job + NULL d_out
    rec.update_dev(0, d_rows.ptr, pos, L)
    same_refusal((capi.CHECK_CORRECT, None, case.dim, d_report.ptr), capi.ERR_STATE, "begin_dev")
    rec.finish_dev(d_out.ptr, case.dim)
    rec.begin_checked_dev(case.indices, pos, L, case.checks)
    rec.update_dev(0, d_rows.ptr, 4, L)
    same_refusal((BAD_POLICY, d_out.ptr, case.dim, d_report.ptr), capi.ERR_STATE, "not fed")              # unfed + policy
    same_refusal((capi.CHECK_CORRECT, d_out.ptr, case.dim, d_report.ptr), capi.ERR_STATE, "not fed", max_errors=3)
    rec.update_dev(4, d_rows.at(4 * L), pos - 4, L)
    same_refusal((BAD_POLICY, d_out.ptr, case.dim, d_report.ptr), capi.ERR_INVALID_ARGUMENT, "max_errors", max_errors=3)
    same_refusal((BAD_POLICY, d_out.ptr, case.dim - 1, d_report.ptr), capi.ERR_INVALID_ARGUMENT, "policy")
    same_refusal((-1, None, case.dim, d_report.ptr), capi.ERR_INVALID_ARGUMENT, "policy")
    same_refusal((capi.CHECK_CORRECT, None, case.dim - 1, d_report.ptr), capi.ERR_INVALID_ARGUMENT, "d_out is NULL")
    same_refusal((capi.CHECK_CORRECT, d_out.ptr, case.dim - 1, None), capi.ERR_INVALID_ARGUMENT, "too small")
    same_refusal((capi.CHECK_CORRECT, d_out.ptr, case.dim, None), capi.ERR_INVALID_ARGUMENT, "d_report is NULL")
    out, report = finish_erasures(rec, case, ec.ok_words(case), True)                                      # ... and the job is intact
    want = ec.model_finish(case, b.rows, ec.CORRECT)
    assert report == want.report and np.array_equal(out, want.out)
    _raises(capi.ERR_STATE, lambda: rec.finish_erasures_dev(0, d_out.ptr, case.dim, d_report.ptr))         # the call ended the job

    # a job of one check: the decoding finish refuses it, this one takes it - but max_errors still has floor(1 / 2) = 0 as its limit
    one = ec.BY_NAME["k3_62-c1-d764-f1-e0-zero"]
    rows = ec.build(one.name).rows
    d_one = DeviceBuffer.from_numpy(np.ascontiguousarray(rows))
    rec.begin_checked_dev(one.indices, pos, rows.shape[1], 1)
    rec.update_dev(0, d_one.ptr, pos, rows.shape[1])
    assert decoded(capi.CHECK_CORRECT, d_out.ptr, one.dim, d_report.ptr) == capi.ERR_INVALID_ARGUMENT and b"one check" in gpu.sda_last_error()
    assert erasures(capi.CHECK_CORRECT, d_out.ptr, one.dim, d_report.ptr, max_errors=1) == capi.ERR_INVALID_ARGUMENT
    assert b"max_errors = 1: 1 checks decode at most 0" in gpu.sda_last_error()
    out, report = finish_erasures(rec, one, ec.ok_words(one), True)
    want = ec.model_finish(one, rows, ec.CORRECT)
    assert report == want.report and np.array_equal(out, want.out) and np.array_equal(out, ec.build(one.name).want)

    # the host form: additive > rows short of t + k > report > policy > max_errors > a short row > out; checks = 1 passes
    pairs = [(i, r) for i, r in zip(case.indices, b.rows)]
    for code, kw in ((capi.ERR_INVALID_ARGUMENT, dict(checks=4, max_errors=3)), (capi.ERR_INVALID_ARGUMENT, dict(checks=5)),
                     (capi.ERR_INVALID_ARGUMENT, dict(checks=1, max_errors=1)), (capi.ERR_INVALID_ARGUMENT, dict(checks=4, erased=[1] * 7)),
                     (capi.ERR_NOT_ENOUGH_SHARES, dict(checks=1, rows=pairs[:3]))):
        with pytest.raises(crypto.SdaError) as e:
            rec.reconstruct_erasures(kw.pop("rows", pairs), **kw)
        assert e.value.code == code, kw
    add = crypto.SecretReconstructor(crypto.Additive(3, vc.SCHEMES[case.scheme][0]), 10)
    with pytest.raises(crypto.SdaError) as e:
        add.reconstruct_erasures([(i, np.zeros(10, dtype=np.int64)) for i in range(3)], checks=2)
    assert e.value.code == capi.ERR_UNSUPPORTED
    idx = (C.c_size_t * pos)(*case.indices)
    n_out = C.c_size_t()
    assert gpu.sda_secret_reconstructor_reconstruct_erasures(rec._h, idx, None, None, pos, 4, None, 0, BAD_POLICY, None, 0, C.byref(n_out),
                                                             None) == capi.ERR_INVALID_ARGUMENT
    assert b"NULL rows" in gpu.sda_last_error()


# ---- 5. the host form ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [ec.E2E, "k3_62-c4-d764-f4-e0-zero", "k3_62-c4-d764-f5-e0-zero", "k3_62-c1-d764-f1-e0-zero",
                                  "k8_62-c16-d805-f8-e4-random", "k3_62-c4-d764-f0-e2-zero-null", "k3_wide-c13-d769-f2-e5-zero"])
def test_reconstruct_erasures_host_form(gpu, name):
    from sda_amd import crypto
    case, b = ec.BY_NAME[name], ec.build(name)
    rec = crypto.SecretReconstructor(scheme_of(case), case.dim)
    pairs = [(i, r) for i, r in zip(case.indices, b.rows)]
    erased = None if case.ok == "null" else [i in case.erased for i in range(len(case.indices))]
    for correct in (False, True):
        want = ec.model_finish(case, b.rows, ec.CORRECT if correct else ec.REPORT)
        vals, dec, f, unrepaired = rec.reconstruct_erasures(pairs, erased, checks=case.checks, max_errors=case.cap, correct=correct)
        assert np.array_equal(vals, want.out)
        assert crypto.RevealDecode.from_words(want.report) == dec and [f, int(unrepaired)] == want.report[6:8]
    if len(case.erased) <= case.checks:
        assert np.array_equal(vals, b.want)
    if case.checks >= 2:                                                  # the sibling host form on the same handle is what it was
        vals, dec = rec.reconstruct_decoded(pairs, checks=case.checks, max_errors=case.cap, correct=True)
        old = dc.Case(name, case.scheme, case.dim, case.indices, case.checks, case.cap, "sums", "none", "one", 0)
        want = dc.model_finish(old, b.rows, dc.CORRECT)
        assert np.array_equal(vals, want.out) and crypto.RevealDecode.from_words(want.report) == dec


# ---- 6. sealed clerking results with tampered boxes ----------------------------------------------------------------------------------
def _boxes(rows, pk, liars, seed):
    from oracle import coracle, sealedbox_oracle as so
    esk = np.random.default_rng(seed).integers(0, 256, size=(len(rows), 32), dtype=np.uint8)
    boxes = [so.seal(coracle.varint_encode(r), pk, e.tobytes()) for r, e in zip(rows, esk)]
    for i in liars:
        boxes[i] = boxes[i][:37] + bytes([boxes[i][37] ^ 0x40]) + boxes[i][38:]                  # one bit of the tag
    return boxes


@pytest.mark.parametrize("name,liars", [("k3_62-c4-d764-f0-e0-zero-ones", (5,)), ("k3_62-c4-d764-f0-e0-zero-ones", (0, 2, 6, 7)),
                                        ("k8_62-c16-d805-f0-e3-zero-ones", (11,)),
                                        ("k8_62-c16-d805-f0-e3-zero-ones", tuple(range(1, 26, 2))[:13] + (0, 2, 4)),
                                        ("k3_wide-c13-d769-f2-e5-zero", (63, 256))])
def test_refused_boxes_are_repaired_from_the_sealed_updates_own_flags(gpu, name, liars):
    """update_sealed_rows_dev refuses the tampered boxes (an ordinary status: bit 16, d_ok[r] = 0); the d_ok array goes to
    finish_erasures_dev as the update left it, and the output is reconstruct() of the other rows.  On config 4's committee the three
    faulty rows of the case are only decodable next to ONE refused box; with f = c = 16 they are taken on trust.  The wide
    committee's 300 boxes go in two calls - d_ok is written at two offsets - and its refused boxes are the case's own erased
    positions, 63 and 256, next to five faulty rows"""
    from sda_amd import crypto
    case = ec.BY_NAME[name]
    b = ec.build(name)
    rows = b.rows if len(liars) < case.checks else b.clean_rows
    assert len(liars) in (1, case.checks) or liars == case.erased
    pk, sk = _keys(61)
    job = upload_boxes(_boxes(rows, pk, liars, 62))
    rec = crypto.SecretReconstructor(scheme_of(case), case.dim)
    f = Feeder(rec, rows, job, pk, sk)
    rec.begin_checked_dev(case.indices, f.pos, f.row_len, case.checks)
    if f.pos <= 256:
        f.feed("one")
    else:                                                                 # the wide committee: the second half first
        half = f.pos // 2
        f.sealed(half, f.pos - half)
        f.sealed(0, half)
    before = u32(f.d_ok, f.pos)
    from sda_amd.device import DeviceBuffer
    d_out = DeviceBuffer.from_numpy(np.full(case.dim + 8, SENTINEL, dtype=np.int64))
    d_report = DeviceBuffer.from_numpy(np.full(ec.HEAD + f.pos + 4, SENTINEL, dtype=np.int64))
    rec.finish_erasures_dev(f.d_ok.ptr, d_out.ptr, case.dim, d_report.ptr, 0, True)
    out, report = d_out.to_numpy(), [int(x) for x in d_report.to_numpy()[:ec.HEAD + f.pos].view(np.uint64)]
    assert f.status() == 16
    assert np.array_equal(u32(f.d_ok, f.pos), before) and [int(i) for i in np.flatnonzero(before == 0)] == sorted(liars)
    assert (out[case.dim:] == SENTINEL).all()
    zeroed = rows.copy()
    zeroed[list(liars)] = 0
    as_flags = case._replace(erased=tuple(sorted(liars)), ok="flags")
    want = ec.model_finish(as_flags, zeroed, ec.CORRECT)
    print("status", f.status(), "report", report[:ec.HEAD])
    assert report == want.report and np.array_equal(out[:case.dim], want.out)
    assert report[6:8] == [len(liars), 0] and report[4] == ec.NONE64
    faulty = b.faulty[0] if rows is b.rows else ()
    keep = [i for i in range(f.pos) if i not in liars and i not in faulty]
    others = crypto.SecretReconstructor(scheme_of(case), case.dim).reconstruct([(case.indices[i], rows[i]) for i in keep])
    assert np.array_equal(out[:case.dim], others) and np.array_equal(others, b.want)


@pytest.mark.parametrize("liars", [(6,), (0, 3, 5, 7)], ids=["one", "f=c"])
def test_reveal_sealed_repaired(gpu, liars):
    """participate_sealed -> clerk_sealed_job per clerk -> some clerking results are tampered with on the way -> reveal_sealed and
    reveal_sealed_decoded fail the reveal (sodium.rs:78-80), reveal_sealed_repaired gives the sum of the inputs, the status word
    with bit 16 and the number of refused boxes"""
    from sda_amd import capi, crypto
    p, k, t, n, w2, w3 = vc.SCHEMES["k3_62"]
    dim, P = 764, 3
    sharing = crypto.PackedShamir(k, n, t, p, w2, w3)
    agg = crypto.Aggregation(dim, p, crypto.Full(p), sharing)
    rng = np.random.default_rng(63)
    secrets = rng.integers(0, p, size=(P, dim), dtype=np.int64)
    truth = (secrets.astype(object).sum(axis=0) % p).astype(np.int64)
    rpk, rsk = _keys(64)
    clerks = [_keys(70 + c) for c in range(n)]
    mask_job, clerk_jobs = crypto.participate_sealed(agg, secrets, rpk, [pk for pk, _ in clerks])
    comb = crypto.ShareCombiner(sharing)
    B = -(-dim // k)
    boxes = [bytes(comb.clerk_sealed_job(clerk_jobs[c], cpk, csk, rpk, B)) for c, (cpk, csk) in enumerate(clerks)]
    for i in liars:
        boxes[i] = boxes[i][:37] + bytes([boxes[i][37] ^ 0x40]) + boxes[i][38:]
    result_job = bytes(crypto.JobContainer.build(0, boxes))
    indices = list(range(n))
    for strict in (lambda: crypto.reveal_sealed(agg, mask_job, result_job, indices, rpk, rsk),
                   lambda: crypto.reveal_sealed_decoded(agg, mask_job, result_job, indices, rpk, rsk, correct=True)):
        with pytest.raises(crypto.SdaError) as e:
            strict()
        assert e.value.code == capi.ERR_SODIUM_DECRYPTION
    got = crypto.reveal_sealed_repaired(agg, mask_job, result_job, indices, rpk, rsk)
    assert got.status & 16 and got.refused == len(liars) and not got.unrepaired
    assert got.decode.bad == 0 and got.decode.blame == (0,) * n and got.decode.first_undecoded is None
    assert np.array_equal(got.output.values, truth)
