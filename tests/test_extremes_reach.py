"""Reach checks for the crafted operands of tests/test_extremes_gpu.py (CPU): run through the models, the crafted batches of
every GPU case (the same batch counts) must push that family's intermediates to a stated fraction of their bounds, measured
against the constants the kernel holds - so a later edit that makes the inputs benign, or crafts them against the wrong
constants, fails here and not silently on the GPU box.
  * mfma: some Toeplitz column >= half of the largest magnitude the digit ranges allow at that term count, and some
    |X| >= half of (k + t) ((p - 1)/2)^2 (2 p^2 at sixteen terms); with the device CSPRNG's random draws, the k crafted
    secrets alone reach 2/5 of the column bound at k terms;
  * l31 / l31_global: the radix of the constants and the group mode are the library's own (sda_debug_select_path), some
    |X| >= half of (k + t) ((p - 1)/2)^2 and some limb column (sum m0 v0 or sum m1 v1) >= half of (k + t) 2^60;
  * generic / mont64 (unsigned canonical products): some sum of canonical constant x canonical value >= half of
    (k + t) (p - 1)^2;
  * n31: some group sum >= half of (terms in the group) ((p - 1)/2)^2, the bound that GROUP p < 2^33 keeps below 2^62
    (a quarter for k + t = 2: two rows of two constants);
  * ngemm: some column at half of what the digit ranges allow at k + t terms (the bounds of tests/test_ngemm_model.py at this
    term count) and some epilogue sum at an eighth of sum_j max |C_j| |c_j|."""
import pytest

import extremes as X


@pytest.fixture(scope="module", autouse=True)
def _oracle():
    from oracle import coracle
    coracle.build()


def _systematic_maps(t):
    return (False, True) if t > 0 else (False,)


def _cases(*families):
    return sorted({(f, k, t, n, p, B) for f, k, t, n, p, _, B, _ in X.GPU_CASES if f in families})


@pytest.mark.parametrize("f,k,t,n,p,B", _cases("mfma"))
def test_mfma_crafted_operands_reach_the_bounds(f, k, t, n, p, B):
    w2, w3 = X.omegas(p, k, t, n)
    for systematic in _systematic_maps(t):
        M = X.share_matrix(p, k, t, n, w2, w3, systematic)
        C = X.family_constants("mfma", M, p)
        vals = X.crafted_rows("mfma", C, p, B, 0, k if systematic else k + t)
        stats = {}
        for b, v in enumerate(vals):
            r = X.target("mfma", b, len(M))[1]
            full = [x % p for x in v] + [0] * (k + t - len(v))        # CSPRNG calls: the draws are not ours (zero here)
            X.mfma_share(M[r], full, p, stats)
        terms = len(vals[0])
        if not systematic:
            assert stats["col"] * 2 >= X.column_bound(terms, p), (stats, X.column_bound(terms, p))
            assert stats["X"] * 2 >= terms * ((p - 1) // 2) ** 2, stats
        else:                   # device CSPRNG: only the k secrets are ours, the draws are random (zero in this model)
            assert stats["col"] * 5 >= X.column_bound(terms, p) * 2, (stats, X.column_bound(terms, p))


@pytest.mark.parametrize("f,k,t,n,p,B", _cases("l31", "l31_global"))
def test_l31_crafted_operands_reach_the_bounds(f, k, t, n, p, B):
    import __graft_entry__ as ge
    ge.build()
    from test_path_select import select
    from sda_amd import capi
    w2, w3 = X.omegas(p, k, t, n)
    got = select(capi.hooks_library(), k, t, n, p, w2, w3)
    assert got["wide"] == f and int(got["l31_radix"]) == X.l31_radix(f, k, t), got       # the constants the kernel holds
    # the group mode these omegas give: (8, 2) runs its one-group Karatsuba form (2), (8, 7) the groups of seven (0)
    assert int(got["l31_group"]) == {(8, 2): 2}.get((k, t), 0), got
    M = X.share_matrix(p, k, t, n, w2, w3)
    C = X.family_constants(f, M, p, k, t)
    vals = X.crafted_rows(f, C, p, B)
    h, kt = (p - 1) // 2, k + t
    best_X = best_col = 0
    for b, v in enumerate(vals):
        row = C[X.target(f, b, len(M))[1]]
        best_X = max(best_X, abs(sum(m * x for m, x in zip(row, v))))
        lm = [X.l31_limbs(m) for m in row]
        lv = [X.l31_limbs(x) for x in v]
        best_col = max(best_col, abs(sum(a[1] * c[1] for a, c in zip(lm, lv))), abs(sum(a[0] * c[0] for a, c in zip(lm, lv))))
    assert best_X * 2 >= kt * h * h, best_X / (kt * h * h)
    assert best_col * 2 >= kt << 60, best_col / (kt << 60)


@pytest.mark.parametrize("f,k,t,n,p,B", _cases("generic", "mont64"))
def test_unsigned_families_crafted_operands_reach_the_bound(f, k, t, n, p, B):
    w2, w3 = X.omegas(p, k, t, n)
    M = X.share_matrix(p, k, t, n, w2, w3)
    Mm = [[m * (1 << 64) % p for m in row] for row in M]                     # Montgomery form, canonical
    vals = X.crafted_rows(f, X.family_constants(f, M, p), p, B)
    best = max(sum(m * (x % p) for m, x in zip(Mm[X.target(f, b, len(M))[1]], v)) for b, v in enumerate(vals))
    assert best * 2 >= (k + t) * (p - 1) ** 2, best / ((k + t) * (p - 1) ** 2)


@pytest.mark.parametrize("f,k,t,n,p,B", _cases("n31"))
def test_n31_crafted_operands_reach_the_group_bound(f, k, t, n, p, B):
    w2, w3 = X.omegas(p, k, t, n)
    M = X.share_matrix(p, k, t, n, w2, w3)
    C = X.family_constants("n31", M, p)
    vals = X.crafted_rows("n31", C, p, B)
    h = (p - 1) // 2
    best = 0.0
    for b, v in enumerate(vals):
        for S, terms in X.n31_group_sums(C[X.target("n31", b, len(M))[1]], v, p):
            best = max(best, abs(S) / (terms * h * h))
    assert best >= (0.5 if k + t >= 4 else 0.25), best        # (1, 1, 2): two rows of two constants, a quarter


@pytest.mark.parametrize("f,k,t,n,p,B", _cases("ngemm"))
def test_ngemm_crafted_operands_reach_the_column_and_epilogue_bounds(f, k, t, n, p, B):
    w2, w3 = X.omegas(p, k, t, n)
    M = X.share_matrix(p, k, t, n, w2, w3)
    C = X.ngemm_constants(M, p)
    kt = k + t
    vals = X.crafted_rows("ngemm", C, p, B)
    h = (p - 1) // 2
    dm = [max(abs(X.ngemm_digits(x)[i]) for x in (h, -h, h - 128, -h + 128)) for i in range(3)]
    dm = [128 if i < 2 else d for i, d in enumerate(dm)]                        # values: canonical residues, digits 0, 1 full
    dv = [128, 128, max(abs(X.ngemm_digits(p - 1)[2]), 1)]
    colb = [kt * sum(dm[a] * dv[c - a] for a in range(3) if 0 <= c - a <= 2) for c in range(5)]
    cj = [abs(X.centred((1 << 32) * 256 ** j % p, p)) for j in range(5)]
    best_col, best_S = [0] * 5, 0
    for b, v in enumerate(vals):
        col, _ = X.ngemm_columns(C[X.target("ngemm", b, len(M))[1]], [x % p for x in v], p)   # every column and C_3 + 256 C_4 fit 32 bits
        best_col = [max(a, abs(c)) for a, c in zip(best_col, col)]
        best_S = max(best_S, abs(sum(c * X.centred((1 << 32) * 256 ** j % p, p) for j, c in enumerate(col))))
    assert max(c / b for c, b in zip(best_col, colb)) >= 0.5, (best_col, colb)
    assert best_S * 2 >= min(sum(b * c for b, c in zip(colb, cj)), p << 31) // 4, best_S
