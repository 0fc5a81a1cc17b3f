"""The decoding finish of the checked reveal on the GPU: sda_secret_reconstructor_finish_decoded_dev / reconstruct_decoded and the
Python chains on top.  Every case of tests/reveal_decode_cases.py runs through update_dev, through update_sealed_rows_dev and
through the mixed feed under both policies; output and every report word are bit-exact against the Python-integer model (proven
to be the definition by tests/test_reveal_decode_reach.py), and finish_checked_dev on the same handle and rows still gives what
reveal_check_cases.model_finish says.  Then the refusals, two tampered boxes of eight, the convenience forms end to end and one
handle across decoded, checked and plain jobs."""
import numpy as np
import pytest

import reveal_check_cases as vc
import reveal_decode_cases as dc
from test_reveal_check_gpu import Feeder, _keys, _raises, finish_checked, run_unchecked, scheme_of, seal_rows, u32, upload_boxes

pytestmark = pytest.mark.gpu
SENTINEL = 0x5A5A5A5A5A5A5A5A
FINISH = b"reveal_decode_finish_kernel"


def finish_decoded(rec, case, correct, max_errors=None):
    """finish_decoded_dev into sentinel-framed buffers: the report buffer starts as garbage (the call initialises it itself)"""
    from sda_amd import capi
    from sda_amd.device import DeviceBuffer
    pos = len(case.indices)
    d_out = DeviceBuffer.from_numpy(np.full(case.dim + 8, SENTINEL, dtype=np.int64))
    d_report = DeviceBuffer.from_numpy(np.full(dc.HEAD + pos + 4, SENTINEL, dtype=np.int64))
    rec.finish_decoded_dev(d_out.ptr, case.dim, d_report.ptr, case.cap if max_errors is None else max_errors, correct)
    assert capi.load().sda_debug_last_kernel() == FINISH
    got, rep = d_out.to_numpy(), d_report.to_numpy()
    assert (got[case.dim:] == SENTINEL).all(), "finish_decoded_dev wrote past its output"
    assert (rep[dc.HEAD + pos:] == SENTINEL).all(), "finish_decoded_dev wrote past its report"
    return got[:case.dim], [int(x) for x in rep[:dc.HEAD + pos].view(np.uint64)]


def run_decoded(case, rows, job, pk, sk, how, correct, rec=None):
    from sda_amd import crypto
    rec = rec or crypto.SecretReconstructor(scheme_of(case), case.dim)
    f = Feeder(rec, rows, job, pk, sk)
    rec.begin_checked_dev(case.indices, f.pos, f.row_len, case.checks)
    note = f.feed(how)
    out, report = finish_decoded(rec, case, correct)
    assert f.status() == 0
    return out, report, note


# ---- 1. every case, every feed, both policies --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in dc.CASES])
def test_case_equals_the_model(gpu, name):
    from sda_amd import crypto
    case, b = dc.BY_NAME[name], dc.build(name)
    pk, sk = _keys(41)
    job = seal_rows(b.rows, pk)
    plain_job = run_unchecked(case, b.rows)
    path = f"sbox_poly_kernel + sealed_stream_weighted_kernel<8, {dc.coef_path(case)}>"
    rec = crypto.SecretReconstructor(scheme_of(case), case.dim)
    for correct in (False, True):
        want = dc.model_finish(case, b.rows, dc.CORRECT if correct else dc.REPORT)
        for how in ("plain", case.feed, "mixed"):
            out, report, note = run_decoded(case, b.rows, job, pk, sk, how, correct, rec=rec)
            bad = int((out != want.out).sum())
            print(f"{name} {'correct' if correct else 'report'} {how}: report {report[:dc.HEAD]} model {want.report[:dc.HEAD]}, "
                  f"output mismatches {bad}, kernel {note}")
            assert report == want.report, (how, correct)
            assert np.array_equal(out, want.out), (how, correct)
            if note is not None:
                assert note == path
            if not correct:
                assert np.array_equal(out, plain_job), "SDA_CHECK_REPORT differs from the unchecked job on the same rows"
        # the sibling finish, on the same handle and rows, is what it was
        f = Feeder(rec, b.rows, job, pk, sk)
        rec.begin_checked_dev(case.indices, f.pos, f.row_len, case.checks)
        f.feed("plain")
        out, report = finish_checked(rec, case, correct)
        old = vc.model_finish(case, b.rows, vc.CORRECT if correct else vc.REPORT)
        assert report == old.report and np.array_equal(out, old.out), "finish_checked_dev changed"
    e = dc.cap_of(case)
    if b.faulty is not None and len(set(b.faulty)) == 1 and 1 <= len(b.faulty[0]) <= e:
        keep = [i for i in range(len(case.indices)) if i not in b.faulty[0]]
        others = crypto.SecretReconstructor(scheme_of(case), case.dim).reconstruct([(case.indices[i], b.rows[i]) for i in keep])
        out, report, _ = run_decoded(case, b.rows, job, pk, sk, "plain", True)
        assert report[1] == report[2] == report[0] > 0 and report[5] == len(b.faulty[0])
        assert np.array_equal(out, others), "SDA_CHECK_CORRECT differs from reconstruct() of the other rows"
        assert np.array_equal(out, b.want)


# ---- 2. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_job_usable(gpu):
    from sda_amd import capi, crypto
    from sda_amd.device import DeviceBuffer
    case, b = dc.BY_NAME[dc.E2E], dc.build(dc.E2E)
    pk, sk = _keys(42)
    job = seal_rows(b.rows, pk)
    L, pos = b.row_len, len(case.indices)
    want = dc.model_finish(case, b.rows, dc.CORRECT)
    d_out, d_report = DeviceBuffer(case.dim + 1), DeviceBuffer(dc.HEAD + pos)
    rec = crypto.SecretReconstructor(scheme_of(case), case.dim)
    f = Feeder(rec, b.rows, job, pk, sk)
    fin = gpu.sda_secret_reconstructor_finish_decoded_dev
    _raises(capi.ERR_STATE, lambda: rec.finish_decoded_dev(d_out.ptr, case.dim, d_report.ptr))       # before any begin
    rec.begin_checked_dev(case.indices, pos, L, case.checks)
    f.sealed(0, 3)
    _raises(capi.ERR_STATE, lambda: rec.finish_decoded_dev(d_out.ptr, case.dim, d_report.ptr))       # positions 3 .. 7 unfed
    f.plain(3, pos - 3)
    _raises(capi.ERR_INVALID_ARGUMENT, lambda: rec.finish_decoded_dev(d_out.ptr, case.dim, d_report.ptr, max_errors=3))   # > 4 / 2
    _raises(capi.ERR_INVALID_ARGUMENT, lambda: rec.finish_decoded_dev(d_out.ptr, case.dim - 1, d_report.ptr))
    _raises(capi.ERR_INVALID_ARGUMENT, lambda: rec.finish_decoded_dev(0, case.dim, d_report.ptr))
    _raises(capi.ERR_INVALID_ARGUMENT, lambda: rec.finish_decoded_dev(d_out.ptr, case.dim, 0))
    assert fin(rec._h, 0, 2, d_out.ptr, case.dim, d_report.ptr, None) == capi.ERR_INVALID_ARGUMENT                        # unknown policy
    assert fin(rec._h, 0, -1, d_out.ptr, case.dim, d_report.ptr, None) == capi.ERR_INVALID_ARGUMENT
    out, report = finish_decoded(rec, case, True)                                                    # ... and the job is intact
    assert report == want.report and np.array_equal(out, want.out)
    _raises(capi.ERR_STATE, lambda: rec.finish_decoded_dev(d_out.ptr, case.dim, d_report.ptr))       # the call ended the job

    # a job with one check decodes nothing: refused, and finish_checked_dev still ends it
    one = case._replace(checks=1)
    rec.begin_checked_dev(case.indices, pos, L, 1)
    f.plain(0, pos)
    _raises(capi.ERR_INVALID_ARGUMENT, lambda: rec.finish_decoded_dev(d_out.ptr, case.dim, d_report.ptr))
    _raises(capi.ERR_INVALID_ARGUMENT, lambda: rec.finish_decoded_dev(d_out.ptr, case.dim, d_report.ptr, max_errors=1))
    out, report = finish_checked(rec, one, True)
    old = vc.model_finish(one, b.rows, vc.CORRECT)
    assert report == old.report and np.array_equal(out, old.out)

    # a plain job refuses the decoding finish and is left intact by it
    rec.begin_dev(case.indices, pos, L)
    f.plain(0, 2)
    _raises(capi.ERR_STATE, lambda: rec.finish_decoded_dev(d_out.ptr, case.dim, d_report.ptr))
    f.sealed(2, pos - 2)
    _raises(capi.ERR_STATE, lambda: rec.finish_decoded_dev(d_out.ptr, case.dim, d_report.ptr))
    rec.finish_dev(d_out.ptr, case.dim)
    assert np.array_equal(d_out.to_numpy()[:case.dim], dc.model_finish(case, b.rows, dc.REPORT).out)
    assert f.status() == 0

    # the host form's own refusals
    pairs = [(i, r) for i, r in zip(case.indices, b.rows)]
    for kw in (dict(checks=1), dict(checks=4, max_errors=3), dict(checks=5), dict(checks=3, max_errors=2)):
        with pytest.raises(crypto.SdaError) as e:
            rec.reconstruct_decoded(pairs, **kw)
        assert e.value.code == capi.ERR_INVALID_ARGUMENT, kw
    add = crypto.SecretReconstructor(crypto.Additive(3, vc.SCHEMES[case.scheme][0]), 10)
    with pytest.raises(crypto.SdaError) as e:
        add.reconstruct_decoded([(i, np.zeros(10, dtype=np.int64)) for i in range(3)], checks=2)
    assert e.value.code == capi.ERR_UNSUPPORTED


def test_refusal_order_is_the_parents(gpu):
    """calls that carry two or three faults at once: which one is reported is part of the interface.  Both device finishes refuse
    in the order  no job > plain job > unfed positions > (decoded: one check > max_errors) > policy > d_out > out_cap > d_report,
    the host forms in the order  additive > rows short of t + k > report > policy > (decoded: checks, max_errors) > a short row >
    out.  Every refused call leaves the job to finish with the model's output."""
    import ctypes as C
    from sda_amd import capi, crypto
    from sda_amd.device import DeviceBuffer
    case, b = dc.BY_NAME[dc.E2E], dc.build(dc.E2E)
    pk, sk = _keys(49)
    L, pos = b.row_len, len(case.indices)
    assert pos == 8 and case.checks == 4
    d_out, d_report = DeviceBuffer(case.dim + 1), DeviceBuffer(dc.HEAD + pos)
    rec = crypto.SecretReconstructor(scheme_of(case), case.dim)
    f = Feeder(rec, b.rows, None, pk, sk)
    checked = lambda policy, out, cap, report, max_errors=None: gpu.sda_secret_reconstructor_finish_checked_dev(
        rec._h, policy, out, cap, report, None)
    decoded = lambda policy, out, cap, report, max_errors=0: gpu.sda_secret_reconstructor_finish_decoded_dev(
        rec._h, max_errors, policy, out, cap, report, None)

    def refused(status, code, word):
        text = gpu.sda_last_error().decode()
        assert status == code and word in text, (status, text, code, word)

    BAD_POLICY = 7
    # a plain job + NULL d_out: the kind of the job comes first
    rec.begin_dev(case.indices, pos, L)
    f.plain(0, pos)
    for fin in (checked, decoded):
        refused(fin(capi.CHECK_CORRECT, None, case.dim, d_report.ptr), capi.ERR_STATE, "begin_dev")
    rec.finish_dev(d_out.ptr, case.dim)
    assert np.array_equal(d_out.to_numpy()[:case.dim], dc.model_finish(case, b.rows, dc.REPORT).out)

    # the checked job of four checks, half fed
    rec.begin_checked_dev(case.indices, pos, L, case.checks)
    f.plain(0, 4)
    for fin in (checked, decoded):
        refused(fin(BAD_POLICY, d_out.ptr, case.dim, d_report.ptr), capi.ERR_STATE, "not fed")                  # unfed + policy
    refused(decoded(capi.CHECK_CORRECT, d_out.ptr, case.dim, d_report.ptr, max_errors=3), capi.ERR_STATE, "not fed")   # unfed + max_errors
    f.plain(4, pos - 4)
    for fin in (checked, decoded):
        refused(fin(BAD_POLICY, d_out.ptr, case.dim - 1, d_report.ptr), capi.ERR_INVALID_ARGUMENT, "policy")    # policy + short out_cap
        refused(fin(capi.CHECK_CORRECT, d_out.ptr, case.dim - 1, None), capi.ERR_INVALID_ARGUMENT, "too small")  # short out_cap + NULL report
    refused(decoded(BAD_POLICY, d_out.ptr, case.dim, d_report.ptr, max_errors=3), capi.ERR_INVALID_ARGUMENT, "max_errors")
    out, report = finish_decoded(rec, case, True)
    want = dc.model_finish(case, b.rows, dc.CORRECT)
    assert report == want.report and np.array_equal(out, want.out)

    # a job of one check + an unknown policy: the decoding finish names the check count
    one = case._replace(checks=1)
    rec.begin_checked_dev(case.indices, pos, L, 1)
    f.plain(0, pos)
    refused(decoded(BAD_POLICY, d_out.ptr, case.dim, d_report.ptr), capi.ERR_INVALID_ARGUMENT, "one check")
    refused(checked(BAD_POLICY, d_out.ptr, case.dim - 1, d_report.ptr), capi.ERR_INVALID_ARGUMENT, "policy")
    out, report = finish_checked(rec, one, True)
    old = vc.model_finish(one, b.rows, vc.CORRECT)
    assert report == old.report and np.array_equal(out, old.out)

    # the host forms
    def host(r, which, rows, checks, policy, with_report, max_errors=0):
        arrs = [np.ascontiguousarray(x, dtype=np.int64) for x in rows]
        idx = (C.c_size_t * len(arrs))(*case.indices[:len(arrs)])
        ptrs = (capi.c_i64p * len(arrs))(*[a.ctypes.data_as(capi.c_i64p) for a in arrs])
        lens = (C.c_size_t * len(arrs))(*[a.size for a in arrs])
        out, n_out = np.empty(case.dim, dtype=np.int64), C.c_size_t()
        words = (C.c_uint64 * (dc.HEAD + len(arrs)))() if with_report else None
        tail = (policy, out.ctypes.data_as(capi.c_i64p), case.dim, C.byref(n_out), words)
        if which == "checked":
            return gpu.sda_secret_reconstructor_reconstruct_checked(r._h, idx, ptrs, lens, len(arrs), checks, *tail)
        return gpu.sda_secret_reconstructor_reconstruct_decoded(r._h, idx, ptrs, lens, len(arrs), checks, max_errors, *tail)

    short = [r for r in b.rows[:-1]] + [b.rows[-1][:dc.batches(case) - 1]]
    add = crypto.SecretReconstructor(crypto.Additive(3, vc.SCHEMES[case.scheme][0]), 10)
    for which in ("checked", "decoded"):
        refused(host(add, which, np.zeros((3, 10), dtype=np.int64), 2, capi.CHECK_REPORT, False), capi.ERR_UNSUPPORTED, "additive")
        refused(host(rec, which, b.rows, 4, BAD_POLICY, False), capi.ERR_INVALID_ARGUMENT, "report is NULL")
        refused(host(rec, which, short, 4, BAD_POLICY, True), capi.ERR_INVALID_ARGUMENT, "policy")
    refused(host(rec, "decoded", short, 1, capi.CHECK_REPORT, True), capi.ERR_INVALID_ARGUMENT, "at least 2 checks")
    refused(host(rec, "checked", short, 1, capi.CHECK_REPORT, True), capi.ERR_ASSERTION, "share vector 7 shorter")


# ---- 3. two tampered boxes of eight --------------------------------------------------------------------------------------------------
def _tampered_job(b, pk, liars):
    from oracle import coracle, sealedbox_oracle as so
    esk = np.random.default_rng(43).integers(0, 256, size=(len(b.rows), 32), dtype=np.uint8)
    boxes = [so.seal(coracle.varint_encode(r), pk, e.tobytes()) for r, e in zip(b.rows, esk)]
    for i in liars:
        boxes[i] = boxes[i][:37] + bytes([boxes[i][37] ^ 0x40]) + boxes[i][38:]
    return boxes


def test_two_tampered_boxes_are_the_blamed_positions(gpu):
    """two refused boxes add nothing: status bit 16 is set (the reveal fails, sodium.rs:78-80), both positions are blamed in every
    batch, and the corrected output is the secrets - the other six rows alone give them"""
    from sda_amd import capi, crypto
    name = "k3_62-c4-d1000-none"
    case, b = dc.BY_NAME[name], dc.build(name)
    pk, sk = _keys(44)
    liars = (2, 5)
    boxes = _tampered_job(b, pk, liars)
    job = upload_boxes(boxes)
    rec = crypto.SecretReconstructor(scheme_of(case), case.dim)
    f = Feeder(rec, b.rows, job, pk, sk)
    rec.begin_checked_dev(case.indices, f.pos, f.row_len, case.checks)
    f.feed("one")
    out, report = finish_decoded(rec, case, True)
    zeroed = b.rows.copy()
    zeroed[list(liars)] = 0
    want = dc.model_finish(case, zeroed, dc.CORRECT)
    print("status", f.status(), "report", report[:dc.HEAD], "blame", report[dc.HEAD:])
    assert f.status() == 16
    assert [int(i) for i in np.flatnonzero(u32(f.d_ok, f.pos) == 0)] == list(liars)
    assert report == want.report and np.array_equal(out, want.out)
    B = dc.batches(case)
    assert report[:3] == [B, B, B] and report[5] == 2 and report[8:16] == [0, B, 0, 0, 0, 0, 0, 0]
    assert report[dc.HEAD:] == [B if i in liars else 0 for i in range(f.pos)]
    assert np.array_equal(out, b.want), "the other six rows alone give the secrets"
    # the chains that own their status word still fail the reveal on such a job
    blob = bytes(crypto.JobContainer.build(0, boxes))
    with pytest.raises(crypto.SdaError) as e:
        rec.reconstruct_sealed_job_decoded(blob, case.indices, pk, sk, correct=True)
    assert e.value.code == capi.ERR_SODIUM_DECRYPTION


# ---- 4. the convenience forms, end to end ----------------------------------------------------------------------------------------
def test_reconstruct_decoded_host_form(gpu):
    from sda_amd import crypto
    case, b = dc.BY_NAME[dc.E2E], dc.build(dc.E2E)
    rec = crypto.SecretReconstructor(scheme_of(case), case.dim)
    pairs = [(i, r) for i, r in zip(case.indices, b.rows)]
    for correct in (False, True):
        want = dc.model_finish(case, b.rows, dc.CORRECT if correct else dc.REPORT)
        vals, dec = rec.reconstruct_decoded(pairs, checks=case.checks, correct=correct)
        assert np.array_equal(vals, want.out)
        assert crypto.RevealDecode.from_words(want.report) == dec and not dec.clean
    vals, dec = rec.reconstruct_decoded(pairs, correct=True)                                 # checks=None: min(r, 4) = 4
    B = dc.batches(case)
    assert np.array_equal(vals, b.want) and dec.most == 2 and dec.by_count[1] == B and dec.first_undecoded is None
    assert {i for i, n in enumerate(dec.blame) if n} == set(b.faulty[0]) and all(dec.blame[i] == B for i in b.faulty[0])
    vals, dec = rec.reconstruct_decoded(pairs, max_errors=1, correct=True)                   # a lowered cap refuses the two rows
    assert dec.decoded == 0 and dec.bad == B and dec.first_undecoded == 0 and not np.array_equal(vals, b.want)
    vals, dec = rec.reconstruct_decoded([(i, r) for i, r in zip(case.indices, b.clean_rows)])
    assert dec.clean and dec.first_bad is None and np.array_equal(vals, b.want)
    assert gpu.sda_reconstruct_decode_report_words(8) == 24


def test_reconstruct_sealed_job_decoded(gpu):
    from sda_amd import crypto
    case, b = dc.BY_NAME[dc.E2E], dc.build(dc.E2E)
    pk, sk = _keys(45)
    enc = crypto.ShareEncryptor(pk)
    job = crypto.JobContainer.build(0, [enc.encrypt(row) for row in b.rows])
    rec = crypto.SecretReconstructor(scheme_of(case), case.dim)
    vals, dec = rec.reconstruct_sealed_job_decoded(bytes(job), case.indices, pk, sk, correct=True)
    want = dc.model_finish(case, b.rows, dc.CORRECT)
    assert np.array_equal(vals, b.want) and np.array_equal(vals, want.out)
    assert crypto.RevealDecode.from_words(want.report) == dec
    vals, dec = rec.reconstruct_sealed_job_decoded(bytes(job), case.indices, pk, sk, checks=2)
    want = dc.model_finish(case._replace(checks=2), b.rows, dc.REPORT)
    assert np.array_equal(vals, want.out) and dec.corrected == 0 and crypto.RevealDecode.from_words(want.report) == dec


@pytest.mark.parametrize("masking", ["full", "none"])
def test_reveal_sealed_decoded_with_two_faulty_clerks(gpu, masking):
    """participate_sealed -> clerk_sealed_job per clerk -> two clerks return wrong sums -> reveal_sealed_decoded: the plain reveal
    is spoiled, the checked one cannot attribute it, the decoded one names both clerks and, corrected, gives the sum of the inputs"""
    from sda_amd import crypto
    p, k, t, n, w2, w3 = vc.SCHEMES["k3_62"]
    dim, P = 1000, 3
    sharing = crypto.PackedShamir(k, n, t, p, w2, w3)
    msch = crypto.Full(p) if masking == "full" else crypto.NoMask()
    agg = crypto.Aggregation(dim, p, msch, sharing)
    rng = np.random.default_rng(46)
    secrets = rng.integers(0, p, size=(P, dim), dtype=np.int64)
    truth = (secrets.astype(object).sum(axis=0) % p).astype(np.int64)
    rpk, rsk = _keys(47)
    clerks = [_keys(50 + c) for c in range(n)]
    mask_job, clerk_jobs = crypto.participate_sealed(agg, secrets, rpk, [pk for pk, _ in clerks])
    comb = crypto.ShareCombiner(sharing)
    B = -(-dim // k)
    sums = []
    for c, (cpk, csk) in enumerate(clerks):
        box = comb.clerk_sealed_job(clerk_jobs[c], cpk, csk, rpk, B)
        sums.append(crypto.ShareDecryptor(rpk, rsk).decrypt(box))
    liars = (1, 6)
    for liar in liars:
        sums[liar] = ((sums[liar].astype(object) + 12345 + liar) % p).astype(np.int64)       # two clerks with a bug
    enc = crypto.ShareEncryptor(rpk)
    result_job = bytes(crypto.JobContainer.build(0, [enc.encrypt(s) for s in sums]))
    indices = list(range(n))
    plain = crypto.reveal_sealed(agg, mask_job, result_job, indices, rpk, rsk)
    assert not np.array_equal(plain.values, truth)
    out, chk = crypto.reveal_sealed_checked(agg, mask_job, result_job, indices, rpk, rsk, correct=True)
    assert chk.bad == B and chk.located == 0 and np.array_equal(out.values, plain.values)
    out, dec = crypto.reveal_sealed_decoded(agg, mask_job, result_job, indices, rpk, rsk)
    assert np.array_equal(out.values, plain.values), "SDA_CHECK_REPORT changes nothing"
    assert dec.bad == dec.decoded == B and dec.corrected == 0 and dec.first_bad == 0 and dec.first_undecoded is None and dec.most == 2
    assert dec.blame == tuple(B if i in liars else 0 for i in range(n))
    out, dec = crypto.reveal_sealed_decoded(agg, mask_job, result_job, indices, rpk, rsk, correct=True)
    assert dec.corrected == B and dec.by_count == (0, B, 0, 0, 0, 0, 0, 0)
    assert np.array_equal(out.values, truth)
    out, dec = crypto.reveal_sealed_decoded(agg, mask_job, result_job, indices, rpk, rsk, max_errors=1, correct=True)
    assert dec.decoded == 0 and dec.first_undecoded == 0 and np.array_equal(out.values, plain.values)


def test_one_handle_across_decoded_checked_and_plain_jobs(gpu):
    from sda_amd import crypto
    from sda_amd.device import DeviceBuffer
    first, second = dc.BY_NAME[dc.E2E], dc.BY_NAME["k3_62-c3-d1000-stair"]
    pk, sk = _keys(48)
    rec = crypto.SecretReconstructor(scheme_of(first), first.dim)
    b1, b2 = dc.build(first.name), dc.build(second.name)
    job1, job2 = seal_rows(b1.rows, pk), seal_rows(b2.rows, pk)
    out, report, _ = run_decoded(first, b1.rows, job1, pk, sk, "one", True, rec=rec)
    want = dc.model_finish(first, b1.rows, dc.CORRECT)
    assert report == want.report and np.array_equal(out, want.out)
    f = Feeder(rec, b1.rows, job1, pk, sk)
    rec.begin_checked_dev(first.indices, f.pos, f.row_len, first.checks)                    # the checked finish on the same rows
    f.feed("mixed")
    out, report = finish_checked(rec, first, True)
    old = vc.model_finish(first, b1.rows, vc.CORRECT)
    assert report == old.report and np.array_equal(out, old.out)
    d_out = DeviceBuffer(first.dim + 1)
    rec.begin_dev(first.indices, f.pos, f.row_len)                                           # a plain job
    f.feed("one")
    rec.finish_dev(d_out.ptr, first.dim)
    assert np.array_equal(d_out.to_numpy()[:first.dim], dc.model_finish(first, b1.rows, dc.REPORT).out)
    out, report, _ = run_decoded(second, b2.rows, job2, pk, sk, "mixed", True, rec=rec)      # other rows, another number of checks
    want = dc.model_finish(second, b2.rows, dc.CORRECT)
    assert report == want.report and np.array_equal(out, want.out)
    vals, dec = rec.reconstruct_decoded([(i, r) for i, r in zip(first.indices, b1.rows)], checks=2)      # the host form in between
    want = dc.model_finish(first._replace(checks=2), b1.rows, dc.REPORT)
    assert np.array_equal(vals, want.out) and crypto.RevealDecode.from_words(want.report) == dec
