"""The reconstructor's CHECKED streaming job on the GPU: sda_secret_reconstructor_begin_checked_dev / finish_checked_dev /
reconstruct_checked.  Every case of tests/reveal_check_cases.py runs through update_dev, through update_sealed_rows_dev and through
the mixed feed under both policies; output and report are bit-exact against the Python-integer model (proven against the C oracle
by tests/test_reveal_check_reach.py), SDA_CHECK_REPORT equals the unchecked job on the same rows, SDA_CHECK_CORRECT on one faulty
position equals reconstruct() of the other rows.  Then the refusals, one handle across jobs of both kinds, a tampered box, and the
three convenience forms end to end."""
import numpy as np
import pytest

import reveal_check_cases as vc

pytestmark = pytest.mark.gpu
SENTINEL = 0x5A5A5A5A5A5A5A5A
FINISH = b"reveal_check_finish_kernel"


def u32(buf, n=1):
    return np.frombuffer(buf.to_bytes(), dtype="<u4")[:n].copy()


def _keys(seed):
    from oracle import sealedbox_oracle as so
    sk = bytes(np.random.default_rng(seed).integers(0, 256, 32, dtype=np.uint8))
    return so.x25519_base(sk), sk


class Job:
    """boxes resident in HBM in the slotted layout: box r at d_boxes + r * slot, lens[r] bytes"""

    def __init__(self, d_boxes, slot, d_lens, rows, keep=()):
        self.d_boxes, self.slot, self.d_lens, self.rows, self.keep = d_boxes, slot, d_lens, rows, keep


def seal_rows(values, pk):
    """every row of `values` varint-encoded and sealed on the device in one call (OS-entropy ephemeral keys)"""
    from sda_amd import crypto
    from sda_amd.device import DeviceBuffer, DeviceBytes, synchronize
    P, L = values.shape
    codec, box = crypto.VarintCodec(), crypto.SealedBox()
    d_v = DeviceBuffer.from_numpy(values)
    slot = max(codec.slot_size(L), 16) + 48
    d_boxes, d_len = DeviceBytes(P * slot).zero(), DeviceBytes(P * 8).zero()
    box.seal_share_rows_dev(codec, [pk], P, d_v.ptr, P, L, L, d_boxes.ptr, slot, d_len.ptr)
    synchronize()
    return Job(d_boxes, slot, d_len, P)


def upload_boxes(boxes):
    """host-made boxes (the oracle's, or tampered ones) as an SDAJOBv1 blob in HBM"""
    from sda_amd import crypto
    from sda_amd.device import DeviceBytes
    job = crypto.JobContainer.build(0, boxes)
    L = job.layout
    d = DeviceBytes.from_bytes(bytes(job))

    class _At:
        def __init__(self, ptr): self.ptr = ptr
    return Job(_At(d.ptr + L.payload_offset), L.slot_bytes, _At(d.ptr + L.lengths_offset), len(boxes), keep=(d,))


def scheme_of(case):
    from sda_amd import crypto
    p, k, t, n, w2, w3 = vc.SCHEMES[case.scheme]
    return crypto.PackedShamir(k, n, t, p, w2, w3)


class Feeder:
    """the updates of one job on `rec`: rows in HBM both decoded and sealed"""

    def __init__(self, rec, rows, job, pk, sk):
        from sda_amd import crypto
        from sda_amd.device import DeviceBuffer, DeviceBytes
        self.rec, self.job, self.pk, self.sk = rec, job, pk, sk
        self.pos, self.row_len = rows.shape
        self.codec, self.box = crypto.VarintCodec(), crypto.SealedBox()
        self.d_rows = DeviceBuffer.from_numpy(rows)
        self.d_status, self.d_ok = DeviceBytes(4).zero(), DeviceBytes(4 * self.pos).zero()

    def sealed(self, first, n):
        j = self.job
        self.rec.update_sealed_rows_dev(self.codec, self.box, self.pk, self.sk, first, j.d_boxes.ptr + first * j.slot, j.slot,
                                        j.d_lens.ptr + 8 * first, n, j.slot, self.d_status.ptr, self.d_ok.ptr + 4 * first)

    def plain(self, first, n):
        self.rec.update_dev(first, self.d_rows.at(first * self.row_len), n, self.row_len)

    def feed(self, how):
        """-> the kernel note of the last sealed update (None: all plaintext)"""
        from sda_amd import capi
        note = None
        if how == "plain":
            self.plain(0, self.pos)
            return None
        if how == "one":
            self.sealed(0, self.pos)
        elif how == "descending":
            for i in reversed(range(self.pos)):
                self.sealed(i, 1)
        else:                                     # mixed: the second half sealed first, then the first half as decoded rows
            h = self.pos // 2
            self.sealed(h, self.pos - h)
            note = capi.load().sda_debug_last_kernel().decode()
            self.plain(0, h)
            return note
        return capi.load().sda_debug_last_kernel().decode()

    def status(self):
        return int(u32(self.d_status)[0])


def finish_checked(rec, case, correct):
    """finish_checked_dev into sentinel-framed buffers: the report buffer starts as garbage (the call initialises it itself)"""
    from sda_amd import capi
    from sda_amd.device import DeviceBuffer
    pos = len(case.indices)
    d_out = DeviceBuffer.from_numpy(np.full(case.dim + 8, SENTINEL, dtype=np.int64))
    d_report = DeviceBuffer.from_numpy(np.full(4 + pos + 4, SENTINEL, dtype=np.int64))
    rec.finish_checked_dev(d_out.ptr, case.dim, d_report.ptr, correct)
    assert capi.load().sda_debug_last_kernel() == FINISH
    got, rep = d_out.to_numpy(), d_report.to_numpy()
    assert (got[case.dim:] == SENTINEL).all(), "finish_checked_dev wrote past its output"
    assert (rep[4 + pos:] == SENTINEL).all(), "finish_checked_dev wrote past its report"
    return got[:case.dim], [int(x) for x in rep[:4 + pos].view(np.uint64)]


def run_checked(case, rows, job, pk, sk, how, correct, rec=None):
    from sda_amd import crypto
    rec = rec or crypto.SecretReconstructor(scheme_of(case), case.dim)
    f = Feeder(rec, rows, job, pk, sk)
    rec.begin_checked_dev(case.indices, f.pos, f.row_len, case.checks)
    note = f.feed(how)
    out, report = finish_checked(rec, case, correct)
    assert f.status() == 0
    return out, report, note


def run_unchecked(case, rows, keep=None):
    """the plain job (begin_dev + update_dev + finish_dev) on positions `keep` of the rows"""
    from sda_amd import crypto
    from sda_amd.device import DeviceBuffer
    keep = list(range(len(case.indices))) if keep is None else keep
    sub = np.ascontiguousarray(rows[keep])
    rec = crypto.SecretReconstructor(scheme_of(case), case.dim)
    d_rows, d_out = DeviceBuffer.from_numpy(sub), DeviceBuffer(case.dim + 1)
    rec.begin_dev([case.indices[i] for i in keep], len(keep), sub.shape[1])
    rec.update_dev(0, d_rows.ptr, len(keep), sub.shape[1])
    rec.finish_dev(d_out.ptr, case.dim)
    return d_out.to_numpy()[:case.dim]


# ---- 1. every case, every feed, both policies --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in vc.CASES])
def test_case_equals_the_model(gpu, name):
    from sda_amd import crypto
    case, b = vc.BY_NAME[name], vc.build(name)
    pk, sk = _keys(21)
    job = seal_rows(b.rows, pk)
    plain_job = run_unchecked(case, b.rows)
    path = f"sbox_poly_kernel + sealed_stream_weighted_kernel<8, {vc.coef_path(case)}>"
    for correct in (False, True):
        want = vc.model_finish(case, b.rows, vc.CORRECT if correct else vc.REPORT)
        for how in ("plain", case.feed, "mixed"):
            out, report, note = run_checked(case, b.rows, job, pk, sk, how, correct)
            bad = int((out != want.out).sum())
            print(f"{name} {'correct' if correct else 'report'} {how}: report {report[:4]} model {want.report[:4]}, output mismatches {bad}, "
                  f"kernel {note}")
            assert report == want.report, (how, correct)
            assert np.array_equal(out, want.out), (how, correct)
            if note is not None:
                assert note == path
            if not correct:
                assert np.array_equal(out, plain_job), "SDA_CHECK_REPORT differs from the unchecked job on the same rows"
    if b.faulty is not None and len(b.faulty) == 1 and case.checks >= 2:
        keep = [i for i in range(len(case.indices)) if i != b.faulty[0]]
        others = crypto.SecretReconstructor(scheme_of(case), case.dim).reconstruct([(case.indices[i], b.rows[i]) for i in keep])
        out, report, _ = run_checked(case, b.rows, job, pk, sk, "plain", True)
        assert report[1] == report[2] > 0
        assert np.array_equal(out, others), "SDA_CHECK_CORRECT differs from reconstruct() of the other rows"


# ---- 2. refusals -----------------------------------------------------------------------------------------------------------------
def _raises(code, call):
    from sda_amd import crypto
    with pytest.raises(crypto.SdaError) as e:
        call()
    assert e.value.code == code, e.value


def test_refusals_leave_a_job_in_flight_usable(gpu):
    from sda_amd import capi, crypto
    from sda_amd.device import DeviceBuffer
    name = "k3_62-c4-d1000-row"
    case, b = vc.BY_NAME[name], vc.build(name)
    pk, sk = _keys(22)
    job = seal_rows(b.rows, pk)
    p, k, t, n, w2, w3 = vc.SCHEMES[case.scheme]
    L, pos = b.row_len, len(case.indices)
    want = vc.model_finish(case, b.rows, vc.CORRECT)
    d_out, d_report = DeviceBuffer(case.dim + 1), DeviceBuffer(4 + pos)

    # additive: no redundancy
    add = crypto.SecretReconstructor(crypto.Additive(3, p), 10)
    _raises(capi.ERR_UNSUPPORTED, lambda: add.begin_checked_dev(None, 3, 10, 1))
    with pytest.raises(crypto.SdaError) as e:
        add.reconstruct_checked([(i, np.zeros(10, dtype=np.int64)) for i in range(3)], checks=1)
    assert e.value.code == capi.ERR_UNSUPPORTED

    rec = crypto.SecretReconstructor(scheme_of(case), case.dim)
    f = Feeder(rec, b.rows, job, pk, sk)
    _raises(capi.ERR_STATE, lambda: rec.finish_checked_dev(d_out.ptr, case.dim, d_report.ptr))       # before any begin
    rec.begin_checked_dev(case.indices, pos, L, case.checks)
    f.sealed(0, 3)

    def refused_begins():
        _raises(capi.ERR_INVALID_ARGUMENT, lambda: rec.begin_checked_dev(case.indices, pos, L, 0))
        _raises(capi.ERR_INVALID_ARGUMENT, lambda: rec.begin_checked_dev(case.indices, pos, L, 5))       # r = 4
        _raises(capi.ERR_INVALID_ARGUMENT, lambda: rec.begin_checked_dev(case.indices, pos, L, 17))      # > SDA_RECONSTRUCT_MAX_CHECKS
        _raises(capi.ERR_INVALID_ARGUMENT, lambda: rec.begin_checked_dev(case.indices[:4], 4, L, 1))     # n_rows == t + k
        _raises(capi.ERR_NOT_ENOUGH_SHARES, lambda: rec.begin_checked_dev(case.indices[:3], 3, L, 1))
        _raises(capi.ERR_ASSERTION, lambda: rec.begin_checked_dev(case.indices, pos, L - 1, 1))
        _raises(capi.ERR_INVALID_ARGUMENT, lambda: rec.begin_checked_dev((0, 1, 2, 3, 4, 5, 6, 0), pos, L, 1))    # colliding
        _raises(capi.ERR_INVALID_ARGUMENT, lambda: rec.begin_checked_dev(None, pos, L, 1))
        _raises(capi.ERR_ASSERTION, lambda: rec.begin_dev(case.indices, pos, L - 1))                    # a refused plain begin too
    refused_begins()
    # the other kind's finishes, on the checked job
    _raises(capi.ERR_STATE, lambda: rec.finish_dev(d_out.ptr, case.dim))
    _raises(capi.ERR_UNSUPPORTED, lambda: crypto.SecretUnmasker(crypto.NoMask()).unmask_jobs_dev(None, rec, d_out.ptr, case.dim))
    _raises(capi.ERR_STATE, lambda: rec.finish_checked_dev(d_out.ptr, case.dim, d_report.ptr))       # positions 3 .. 7 unfed
    f.plain(3, pos - 3)
    _raises(capi.ERR_STATE, lambda: rec.finish_dev(d_out.ptr, case.dim))
    _raises(capi.ERR_UNSUPPORTED, lambda: crypto.SecretUnmasker(crypto.NoMask()).unmask_jobs_dev(None, rec, d_out.ptr, case.dim))
    _raises(capi.ERR_INVALID_ARGUMENT, lambda: rec.finish_checked_dev(d_out.ptr, case.dim - 1, d_report.ptr))
    _raises(capi.ERR_INVALID_ARGUMENT, lambda: rec.finish_checked_dev(0, case.dim, d_report.ptr))
    _raises(capi.ERR_INVALID_ARGUMENT, lambda: rec.finish_checked_dev(d_out.ptr, case.dim, 0))
    assert gpu.sda_secret_reconstructor_finish_checked_dev(rec._h, 2, d_out.ptr, case.dim, d_report.ptr, None) == capi.ERR_INVALID_ARGUMENT
    out, report = finish_checked(rec, case, True)                                                    # ... and the job is intact
    assert report == want.report and np.array_equal(out, want.out)
    _raises(capi.ERR_STATE, lambda: rec.finish_checked_dev(d_out.ptr, case.dim, d_report.ptr))       # the call ended the job

    # a plain job refuses the checked finish and is left intact by it and by refused checked begins
    rec.begin_dev(case.indices, pos, L)
    f.plain(0, 2)
    _raises(capi.ERR_STATE, lambda: rec.finish_checked_dev(d_out.ptr, case.dim, d_report.ptr))
    refused_begins()
    f.sealed(2, pos - 2)
    _raises(capi.ERR_STATE, lambda: rec.finish_checked_dev(d_out.ptr, case.dim, d_report.ptr))
    rec.finish_dev(d_out.ptr, case.dim)
    assert np.array_equal(d_out.to_numpy()[:case.dim], vc.model_finish(case, b.rows, vc.REPORT).out)
    assert f.status() == 0


def test_one_handle_across_checked_and_plain_jobs(gpu):
    """a checked job, an unchecked job, then a checked job with other indices and another number of checks on the same handle"""
    from sda_amd import crypto
    from sda_amd.device import DeviceBuffer
    first, second = vc.BY_NAME["k3_62-c4-d1000-row"], vc.BY_NAME["k3_62-five-c1-d1000-row"]
    pk, sk = _keys(23)
    rec = crypto.SecretReconstructor(scheme_of(first), first.dim)
    b1, b2 = vc.build(first.name), vc.build(second.name)
    job1, job2 = seal_rows(b1.rows, pk), seal_rows(b2.rows, pk)
    out, report, _ = run_checked(first, b1.rows, job1, pk, sk, "one", True, rec=rec)
    want = vc.model_finish(first, b1.rows, vc.CORRECT)
    assert report == want.report and np.array_equal(out, want.out)
    f = Feeder(rec, b1.rows, job1, pk, sk)
    d_out = DeviceBuffer(first.dim + 1)
    rec.begin_dev(first.indices, f.pos, f.row_len)
    f.feed("mixed")
    rec.finish_dev(d_out.ptr, first.dim)
    assert np.array_equal(d_out.to_numpy()[:first.dim], vc.model_finish(first, b1.rows, vc.REPORT).out)
    out, report, _ = run_checked(second, b2.rows, job2, pk, sk, "mixed", True, rec=rec)
    want = vc.model_finish(second, b2.rows, vc.CORRECT)
    assert report == want.report and np.array_equal(out, want.out)
    # the host form on the same handle, in between
    vals, chk = rec.reconstruct_checked([(i, r) for i, r in zip(first.indices, b1.rows)], checks=2)
    want = vc.model_finish(first._replace(checks=2), b1.rows, vc.REPORT)
    assert np.array_equal(vals, want.out) and [chk.bad, chk.located, chk.corrected] == want.report[:3]


def test_a_tampered_box_is_the_blamed_position(gpu):
    """a refused box adds nothing: status bit 16 is set (the reveal fails, sodium.rs:78-80) AND the position is the one blamed"""
    from oracle import coracle, sealedbox_oracle as so
    name = "k3_62-c4-d1000-clean"
    case, b = vc.BY_NAME[name], vc.build(name)
    pk, sk = _keys(24)
    esk = np.random.default_rng(24).integers(0, 256, size=(len(b.rows), 32), dtype=np.uint8)
    boxes = [so.seal(coracle.varint_encode(r), pk, e.tobytes()) for r, e in zip(b.rows, esk)]
    boxes[5] = boxes[5][:37] + bytes([boxes[5][37] ^ 0x40]) + boxes[5][38:]
    job = upload_boxes(boxes)
    from sda_amd import crypto
    rec = crypto.SecretReconstructor(scheme_of(case), case.dim)
    f = Feeder(rec, b.rows, job, pk, sk)
    rec.begin_checked_dev(case.indices, f.pos, f.row_len, case.checks)
    f.feed("one")
    out, report = finish_checked(rec, case, True)
    zeroed = b.rows.copy()
    zeroed[5] = 0
    want = vc.model_finish(case, zeroed, vc.CORRECT)
    print("status", f.status(), "report", report)
    assert f.status() == 16
    assert [int(i) for i in np.flatnonzero(u32(f.d_ok, f.pos) == 0)] == [5]
    assert report == want.report and np.array_equal(out, want.out)
    assert report[0] > 0 and {i for i, n in enumerate(report[4:]) if n} == {5}
    assert np.array_equal(out, b.want), "the other seven rows alone give the secrets"


# ---- 3. the convenience forms, end to end ----------------------------------------------------------------------------------------
def test_reconstruct_checked_host_form(gpu):
    from sda_amd import crypto
    case, b = vc.BY_NAME[vc.E2E], vc.build(vc.E2E)
    rec = crypto.SecretReconstructor(scheme_of(case), case.dim)
    pairs = [(i, r) for i, r in zip(case.indices, b.rows)]
    for correct in (False, True):
        want = vc.model_finish(case, b.rows, vc.CORRECT if correct else vc.REPORT)
        vals, chk = rec.reconstruct_checked(pairs, checks=case.checks, correct=correct)
        assert np.array_equal(vals, want.out)
        assert [chk.bad, chk.located, chk.corrected, chk.first_bad] + list(chk.blame) == want.report
        assert not chk.clean
    vals, chk = rec.reconstruct_checked(pairs, correct=True)                                 # checks=None: min(r, 4) = 4
    assert np.array_equal(vals, b.want) and chk.blame[b.faulty[0]] == vc.batches(case)
    vals, chk = rec.reconstruct_checked([(i, r) for i, r in zip(case.indices, b.clean_rows)])
    assert chk.clean and chk.first_bad is None and np.array_equal(vals, b.want)
    assert gpu.sda_reconstruct_report_words(8) == 12


def test_reconstruct_sealed_job_checked(gpu):
    from sda_amd import capi, crypto
    case, b = vc.BY_NAME[vc.E2E], vc.build(vc.E2E)
    pk, sk = _keys(25)
    enc = crypto.ShareEncryptor(pk)
    job = crypto.JobContainer.build(0, [enc.encrypt(row) for row in b.rows])
    rec = crypto.SecretReconstructor(scheme_of(case), case.dim)
    vals, chk = rec.reconstruct_sealed_job_checked(bytes(job), case.indices, pk, sk, correct=True)
    want = vc.model_finish(case, b.rows, vc.CORRECT)
    assert np.array_equal(vals, b.want) and np.array_equal(vals, want.out)
    assert [chk.bad, chk.located, chk.corrected, chk.first_bad] + list(chk.blame) == want.report
    vals, chk = rec.reconstruct_sealed_job_checked(bytes(job), case.indices, pk, sk, checks=2)
    want = vc.model_finish(case._replace(checks=2), b.rows, vc.REPORT)
    assert np.array_equal(vals, want.out) and chk.corrected == 0 and chk.located == want.report[1]
    bad = bytearray(bytes(job))
    bad[job.layout.payload_offset + 2 * job.layout.slot_bytes + 40] ^= 1
    with pytest.raises(crypto.SdaError) as e:
        rec.reconstruct_sealed_job_checked(bytes(bad), case.indices, pk, sk)
    assert e.value.code == capi.ERR_SODIUM_DECRYPTION


@pytest.mark.parametrize("masking", ["full", "none"])
def test_reveal_sealed_checked_with_one_faulty_clerk(gpu, masking):
    """participate_sealed -> clerk_sealed_job per clerk -> one clerk returns a wrong sum -> reveal_sealed_checked: the plain reveal
    is spoiled, the checked one names the clerk and, corrected, gives the sum of the inputs"""
    from sda_amd import crypto
    p, k, t, n, w2, w3 = vc.SCHEMES["k3_62"]
    dim, P = 1000, 3
    sharing = crypto.PackedShamir(k, n, t, p, w2, w3)
    msch = crypto.Full(p) if masking == "full" else crypto.NoMask()
    agg = crypto.Aggregation(dim, p, msch, sharing)
    rng = np.random.default_rng(26)
    secrets = rng.integers(0, p, size=(P, dim), dtype=np.int64)
    truth = (secrets.astype(object).sum(axis=0) % p).astype(np.int64)
    rpk, rsk = _keys(27)
    clerks = [_keys(30 + c) for c in range(n)]
    mask_job, clerk_jobs = crypto.participate_sealed(agg, secrets, rpk, [pk for pk, _ in clerks])
    comb = crypto.ShareCombiner(sharing)
    B = -(-dim // k)
    sums = []
    for c, (cpk, csk) in enumerate(clerks):
        box = comb.clerk_sealed_job(clerk_jobs[c], cpk, csk, rpk, B)
        sums.append(crypto.ShareDecryptor(rpk, rsk).decrypt(box))
    liar = 6
    sums[liar] = ((sums[liar].astype(object) + 12345) % p).astype(np.int64)                  # a clerk with a bug
    enc = crypto.ShareEncryptor(rpk)
    result_job = bytes(crypto.JobContainer.build(0, [enc.encrypt(s) for s in sums]))
    indices = list(range(n))
    plain = crypto.reveal_sealed(agg, mask_job, result_job, indices, rpk, rsk)
    assert not np.array_equal(plain.values, truth)
    out, chk = crypto.reveal_sealed_checked(agg, mask_job, result_job, indices, rpk, rsk)
    assert np.array_equal(out.values, plain.values), "SDA_CHECK_REPORT changes nothing"
    assert chk.bad == chk.located == B and chk.corrected == 0 and chk.first_bad == 0
    assert chk.blame == tuple(B if i == liar else 0 for i in range(n))
    out, chk = crypto.reveal_sealed_checked(agg, mask_job, result_job, indices, rpk, rsk, checks=2, correct=True)
    assert chk.corrected == B and chk.blame[liar] == B
    assert np.array_equal(out.values, truth)
