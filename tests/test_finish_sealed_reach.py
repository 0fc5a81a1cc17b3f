"""What the case table of sda_share_combiner_finish_sealed_rows_dev (tests/finish_sealed_cases.py) reaches, proved with Python
integers on the CPU: every item the GPU run is meant to exercise is asserted BY NAME here, from the rows the cases feed - so a
case that stopped reaching its target (a changed seed, a changed block size) fails this file instead of silently testing less.
Nothing here skips and nothing is capped: every case must build and every item must be reached."""
import finish_sealed_cases as fc

V = fc.V


def _all_jobs():
    """(case, job index, 128-bit sums from the ROWS, residues, geometry) of every job of the table"""
    out = []
    for c in fc.CASES:
        rows = fc.rows_of(c)
        res = fc.residues_of(c, rows)
        for j in range(c["jobs"]):
            sums = [sum(int(rows[j, r, i]) for r in range(rows.shape[1])) for i in range(c["dim"])]
            out.append((c, j, sums, res[j], fc.geometry(res[j])))
    return out


JOBS = _all_jobs()


def test_the_restated_geometry_is_the_kernels():
    """V, the stage and the keystream tile as sda_amd/csrc/varint_kernels.hip defines them, and the call the table is for"""
    import os
    import re
    from sda_amd import capi
    assert "sda_share_combiner_finish_sealed_rows_dev" in capi.SIGNATURES
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sda_amd", "csrc", "varint_kernels.hip")).read()
    const = {k: v for k, v in re.findall(r"static constexpr int (k\w+) = ([^;]+);", src)}
    assert int(const["kVT"]) * int(const["kVals"]) == V and const["kSumVals"] == "kVT * kVals"
    assert const["kSumStage"] == "64 + kSumVals * 10" and const["kSumKsBlocks"] == "kSumStage / 64"
    assert "sum_len_kernel" in src and "sum_seal_wide_kernel" in src


def test_the_rows_give_the_sums_the_table_asks_for():
    for c, j, sums, res, _ in JOBS:
        assert sums == c["sums"][j], c["name"]
        assert all(0 <= r < c["m"] for r in res)
        assert all(fc.SUM_MIN <= t <= fc.SUM_MAX for t in sums)


def test_every_varint_length_1_to_9_occurs_and_10_cannot():
    seen = {fc.varint_len(r) for _, _, _, res, _ in JOBS for r in res}
    assert seen == set(range(1, 10)), seen
    # a canonical residue is below the modulus, the modulus below 2^62: zig-zag doubles it, so at most 63 bits = 9 bytes
    assert fc.varint_len((1 << 62) - 1) == 9 and fc.varint_len(1 << 62) == 10
    assert all(c["m"] < (1 << 62) for c in fc.CASES)
    # ... and the codec agrees with the length function on every boundary
    from oracle import pyoracle as po
    for L in range(1, 10):
        lo, hi = fc.len_range(L, 1 << 62)
        assert len(po.varint_encode([lo])) == L == len(po.varint_encode([hi])) and fc.varint_len(hi + 1) == L + 1


def test_every_length_boundary_of_every_modulus_is_a_residue_of_its_limits_case():
    for name in ("limits-p62", "limits-433", "limits-additive"):
        c = fc.BY_NAME[name]
        res = set(fc.residues_of(c)[0])
        for L in range(1, 10):
            rng = fc.len_range(L, c["m"])
            if rng:
                assert rng[0] in res and rng[1] in res, (name, L)
    assert fc.max_len(fc.P62) == 9 and fc.max_len(fc.M_ADD) == 9 and fc.max_len(fc.M433) == 2


def test_residues_zero_and_m_minus_one():
    for m in (fc.P62, fc.M433, fc.M_ADD):
        res = {r for c, _, _, rs, _ in JOBS if c["m"] == m for r in rs}
        assert 0 in res and m - 1 in res, m


def test_sums_below_zero_past_2_64_and_on_a_multiple_of_m():
    for m in (fc.P62, fc.M433, fc.M_ADD):
        sums = [t for c, _, ts, _, _ in JOBS if c["m"] == m for t in ts]
        assert any(t < 0 for t in sums), "acc_hi below 0"
        assert any(t >= (1 << 64) for t in sums), "acc_hi above 0"
        assert any(t != 0 and t % m == 0 for t in sums), "a non-zero multiple of m"
        assert any(t < 0 and t % m == 0 for t in sums) and any(t >= (1 << 64) and t % m == 0 for t in sums)
    sums = fc.BY_NAME["limits-p62"]["sums"][0]
    for t in (fc.SUM_MAX, fc.SUM_MIN, 1 << 64, (1 << 64) - 1, -(1 << 64), -1):
        assert t in sums, t
    # the mixed cases lift their sums too: the big rows are not all small positive sums
    big = next(ts for c, _, ts, _, _ in JOBS if c["name"] == "blocks70")
    assert sum(t < 0 for t in big) > 1000 and sum(t >= (1 << 64) for t in big) > 1000


def test_dimensions_around_the_block_size():
    dims = {c["dim"] for c in fc.CASES if c["jobs"] == 1}
    for d in (1, 2, V - 1, V, V + 1, 2 * V, 2 * V + 1):
        assert d in dims, d
    assert len(next(g for c, _, _, _, g in JOBS if c["name"] == "blocks70")) == 70
    assert [len(g) for c, _, _, _, g in JOBS if c["name"] in ("V-1", "V", "V+1", "2V", "2V+1")] == [1, 1, 2, 2, 3]


def test_block_offsets_cover_every_phase():
    g = next(g for c, _, _, _, g in JOBS if c["name"] == "blocks70")
    offs = [off for off, _, _, _ in g]
    assert {o % 64 for o in offs} == set(range(64))
    assert {o % 4 for o in offs} == {0, 1, 2, 3}
    assert {(32 + o) % 64 for o in offs} == set(range(64))                # the stage pad of sum_seal_wide_kernel
    # the device offset is an entry of the scan over ALL jobs minus the entry of the job's first block: the destination phase
    # (boxes are 16-byte aligned, the ciphertext starts at byte 48) is the offset's own
    assert {(48 + o) % 4 for o in offs} == {0, 1, 2, 3}


def test_salsa_blocks_per_workgroup():
    most = 0
    for c, _, _, _, g in JOBS:
        for off, total, first, count in g:
            assert first == (32 + off) // 64
            assert count <= total // 64 + 2
            assert count <= (64 + V * 10) // 64                          # kSumKsBlocks
            most = max(most, count)
    assert most > 256, "no workgroup needs a second Salsa20 block per lane"
    # a block that starts inside a Salsa20 block and one that starts on its edge
    pads = {(32 + off) % 64 for _, _, _, _, g in JOBS for off, _, _, _ in g}
    assert 0 in pads and 63 in pads


def test_rows_around_the_first_salsa_blocks_edge():
    totals = sorted(sum(t for _, t, _, _ in g) for c, _, _, _, g in JOBS if c["name"] == "edge32")
    assert totals == [31, 32, 33]
    assert any(sum(t for _, t, _, _ in g) < 32 for _, _, _, _, g in JOBS)


def test_a_block_of_one_byte_values_and_one_of_nine_byte_values():
    c = fc.BY_NAME["all1-all9"]
    res = fc.residues_of(c)[0]
    assert {fc.varint_len(r) for r in res[:V]} == {1} and {fc.varint_len(r) for r in res[V:2 * V]} == {9}
    g = fc.geometry(res)
    assert g[0][1] == V and g[1][1] == 9 * V and len(g) == 3 and g[1][3] > 256


def test_jobs_1_2_3_with_rows_of_different_lengths():
    assert {c["jobs"] for c in fc.CASES} == {1, 2, 3}
    for name in ("jobs2", "jobs3", "edge32", "433-2V"):
        c = fc.BY_NAME[name]
        totals = [sum(t for _, t, _, _ in fc.geometry(r)) for r in fc.residues_of(c)]
        assert len(set(totals)) == c["jobs"], (name, totals)
        firsts = [e[0] for e in fc.scan_entries(c)]
        assert any(f % 4 for f in firsts[1:]), f"{name}: no job starts its scan entries inside a dword"
    assert {e[0] % 4 for e in fc.scan_entries(fc.BY_NAME["jobs3"])} == {0, 1, 3}
    assert all(len(g) == 2 for c, _, _, _, g in JOBS if c["name"] == "jobs3")       # more than one block per job


def test_moduli():
    ms = {c["m"] for c in fc.CASES}
    assert ms == {fc.P62, fc.M433, fc.M_ADD}
    assert fc.P62.bit_length() == 62 and all(fc.P62 % q for q in (2, 3, 5, 7, 11, 13)) and pow(2, fc.P62 - 1, fc.P62) == 1
    assert fc.M_ADD % 2 == 0 and fc.M_ADD < (1 << 62)
    assert any(c["m"] == fc.M433 and len(fc.geometry(fc.residues_of(c)[0])) > 1 for c in fc.CASES)
    assert any(c["m"] == fc.M_ADD and len(fc.geometry(fc.residues_of(c)[0])) > 1 for c in fc.CASES)


def test_the_reference_opens_to_the_residues():
    from oracle import pyoracle as po, sealedbox_oracle as so
    pk, sk = fc.recipient_keys()
    for name in ("limits-p62", "edge32", "jobs2"):
        c = fc.BY_NAME[name]
        for box, res in zip(fc.oracle_boxes(c), fc.residues_of(c)):
            assert po.varint_decode(so.seal_open(box, pk, sk)) == res
