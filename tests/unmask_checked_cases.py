"""Cases of sda_secret_unmasker_unmask_checked_jobs_dev - the recipient's last step on a CHECKED reconstructor job and a mask
combiner job, in one call - and its Python-integer model, shared by tests/test_unmask_checked_reach.py (which proves on the CPU what
the table contains, that the model is the composition of the existing models, and that a planted fault is noticed by a named case)
and tests/test_unmask_checked_gpu.py (which runs every case against the model and against the three-call chain on twin jobs).

The model.  v = what the named finish stores, from the models whose reach tests prove them to be the definition
(reveal_check_cases.model_finish, reveal_decode_cases.model_finish, reveal_erasure_cases.model_finish - they read a case's scheme,
dim, indices, checks, cap, erased and ok, which a Case here carries under the same names); the mask = Python-integer sums of the
mask rows, or of the seeds' ChaCha masks, folded under q_mask as in unmask_jobs_cases; the stored value (v % q_mask - mask) % q_mask;
the report the finish model's, written whether or not the gate is shut.  Nothing here needs a device; the C oracle is needed by
the borrowed cases alone, whose rows the finish tables build from its shares.

The rows.  Position i holds f_b(x_i) for batch b, f_b = (x - 1) g_b with g_b of degree < t + k drawn per batch: a polynomial of degree
<= t + k that vanishes at the node 1, which is what clean clerk sums are (reveal_check_cases: "The mathematics").  `faulty` whole
rows among the non-erased ones then carry a non-zero error in every batch, the erased rows hold zeros (a refused box adds nothing).
"crafted" rows are any-int64 specials: no polynomial, the model alone says what comes out, and masked values at or above a q_mask
below the sharing modulus occur.

The kernels take one lane per batch, 256 lanes per workgroup, and fold a batch's secrets in groups of up to four: the shapes are one
group of 3 (k3_62, k3_31), 4 + 4 (k8_62) and 25 groups (pss155, dimension 250: 50 padding sums); 1, 255, 256 and 257 batches;
dimension mod k = 0, 1 and 2; d_out on and 8 bytes past a 16-byte boundary.

The wide committees.  The three kernels share the decoder walks with the finish kernels and repeat everything around them: the
syndrome fold, the staging of positions and magnitudes, the correction loops, the table look-ups, every report atomic.  So the
cases the finish tables keep for that glue run here as well, BORROWED: the rows their own build() makes - 300, 257, 256, 65 and 64
rows, faulty and erased rows pinned at and past position 256, steered syndromes in every wave - under both policies and a fixed
rotation of masking arrangements.  Beside them: sparse faults over five workgroups (1100 batches), the guard of the partial group at
every residue of k = 8 and around a group boundary of k = 100, forty mask rows, the smallest and the largest masking modulus, and
three wide cases behind a shut gate.  tests/test_unmask_checked_reach.py prints what they reach."""
import collections
import functools
import zlib

import numpy as np

import chacha_repair as cr
import reconstruct_stream_cases as rc
import reveal_check_cases as vc
import reveal_decode_cases as dc
import reveal_erasure_cases as ec
import unmask_jobs_cases as uc

P62, P31, Q61, TSS_P = rc.P62, rc.P31, uc.Q61, rc.TSS_P
SENTINEL, TAIL = uc.SENTINEL, uc.TAIL
REPORT, CORRECT = vc.REPORT, vc.CORRECT
LOCATE, DECODE, ERASURES = 0, 1, 2            # SDA_CHECKED_END_*
ENDS = {LOCATE: "locate", DECODE: "decode", ERASURES: "erasures"}
KERNELS = {LOCATE: b"reveal_check_unmask_kernel", DECODE: b"reveal_decode_unmask_kernel<false>",
           ERASURES: b"reveal_erasure_setup_kernel + reveal_decode_unmask_kernel<true>"}

# end    : LOCATE | DECODE | ERASURES;  policy: REPORT | CORRECT;  cap: max_errors as passed
# faulty : whole faulty rows among the non-erased ones;  erased: the erased positions (ERASURES; ok = "flags" | "null")
# values : "sums" (clean rows + the faults) | "crafted" (any-int64 rows)
# masking: "full" | "chacha" | "none-null" (c = NULL) | "none-combiner" (a None combiner, begun);  masks as in unmask_jobs_cases
# gates  : "null" | "two" (two words) | "equal" (one word given twice);  word_m / word_r: what the masks' / the results' status word
#          holds when the call is made ("equal": the one word holds both);  pass_bits: results_pass_bits
#
# ... and the fields that came with the wide committees (defaults: a case of the older table says nothing about them):
# source, source_name: values "borrowed" - the rows are those the case `source_name` of the finish table `source` ("reveal_check_cases" |
#          "reveal_decode_cases" | "reveal_erasure_cases") builds, with its scheme, dim, indices, checks, cap, pin, erased, fill and ok
#          ("ones": d_ok of non-zero words)
# pin, fill: the source's, carried for the record (the rows are the source's own)
# bad    : values "sparse" - clean rows everywhere but in the listed batches: ((batch, (positions with an error)), ...)
# masks  : also "crafted40" - 40 any-int64 rows whose 128-bit sums reach high words beyond +-8
Case = collections.namedtuple("Case", "name scheme dim indices checks end policy cap faulty erased ok values masking q_mask masks "
                                      "offset gates word_m word_r pass_bits source source_name pin fill bad",
                              defaults=(None, None, None, "zero", None))
SOURCES = {"reveal_check_cases": vc, "reveal_decode_cases": dc, "reveal_erasure_cases": ec}

ALL8, K8_ALL, PSS_260 = vc.ALL8, vc.K8_ALL, vc.PSS_260


def _cases():
    out = []

    def add(name, scheme, dim, indices, checks, end, policy, faulty=0, erased=(), cap=0, ok="flags", values="sums", masking="full",
            q_mask=P62, masks="random", offset=0, gates="two", word_m=0, word_r=0, pass_bits=0):
        out.append(Case(name, scheme, dim, indices, checks, end, policy, cap, faulty, tuple(sorted(erased)), ok, values, masking, q_mask, masks,
                        offset, gates, word_m, word_r, pass_bits))
    # config 3's committee (8 rows, k = 3, t = 1: one group of 3), 4 checks.  Every end with both policies at 255, 256 and 257
    # batches (dimension mod 3 = 2, 1, 1) with the row sets that end decides: one faulty row; floor(checks / 2) faulty rows; one
    # erased row and one faulty row
    for policy, tag in ((REPORT, "report"), (CORRECT, "correct")):
        add(f"k3_62-locate-{tag}-d769-row1", "k3_62", 769, ALL8, 4, LOCATE, policy, faulty=1, offset=8 * policy, gates="null")
        add(f"k3_62-decode-{tag}-d766-rows2", "k3_62", 766, ALL8, 4, DECODE, policy, faulty=2, offset=8 - 8 * policy)
        add(f"k3_62-erasures-{tag}-d764-f1-e1", "k3_62", 764, ALL8, 4, ERASURES, policy, faulty=1, erased=(5,), offset=8 * policy, gates="equal")
    # clean rows, one batch, every end; then 257 batches with dimension mod 3 = 0
    for end in ENDS:
        add(f"k3_62-{ENDS[end]}-correct-d3-clean", "k3_62", 3, ALL8, 4, end, CORRECT, offset=8 * (end % 2))
        add(f"k3_62-{ENDS[end]}-correct-d771-clean", "k3_62", 771, ALL8, 4, end, CORRECT, masking="chacha", masks="seeds")
    add("k3_62-decode-correct-d1-row1", "k3_62", 1, ALL8, 4, DECODE, CORRECT, faulty=1, offset=8)
    add("k3_62-decode-correct-d2-row1-cap1", "k3_62", 2, ALL8, 4, DECODE, CORRECT, faulty=1, cap=1)
    # one more than the end corrects: stays unlocated / undecoded, stored as it folds
    add("k3_62-locate-correct-d769-rows2", "k3_62", 769, ALL8, 4, LOCATE, CORRECT, faulty=2)
    add("k3_62-decode-correct-d771-rows3", "k3_62", 771, ALL8, 4, DECODE, CORRECT, faulty=3, offset=8)
    add("k3_62-erasures-correct-d764-f2-e2", "k3_62", 764, ALL8, 4, ERASURES, CORRECT, faulty=2, erased=(0, 7))
    # erasures: f = 1, f = checks, f = checks + 1 (report[7] = 1: the plain fold), d_ok NULL
    add("k3_62-erasures-correct-d766-f1", "k3_62", 766, ALL8, 4, ERASURES, CORRECT, erased=(3,), offset=8)
    add("k3_62-erasures-correct-d766-f4", "k3_62", 766, ALL8, 4, ERASURES, CORRECT, erased=(0, 2, 5, 7))
    add("k3_62-erasures-correct-d766-f5", "k3_62", 766, ALL8, 4, ERASURES, CORRECT, erased=(0, 1, 2, 5, 7), offset=8)
    add("k3_62-erasures-correct-d766-null-row1", "k3_62", 766, ALL8, 4, ERASURES, CORRECT, faulty=1, ok="null")
    # k8_62 (26 rows, k = 8, t = 2: groups of 4 + 4), 16 checks, dimension mod 8 = 5: 8 and 9 faulty rows, 16 and 17 erased
    add("k8_62-locate-correct-d61-row1", "k8_62", 61, K8_ALL, 16, LOCATE, CORRECT, faulty=1)
    add("k8_62-decode-correct-d61-rows8", "k8_62", 61, K8_ALL, 16, DECODE, CORRECT, faulty=8, offset=8)
    add("k8_62-decode-correct-d61-rows9", "k8_62", 61, K8_ALL, 16, DECODE, CORRECT, faulty=9)
    add("k8_62-erasures-correct-d61-f16", "k8_62", 61, K8_ALL, 16, ERASURES, CORRECT, erased=tuple(range(1, 17)), masking="chacha", masks="seeds")
    add("k8_62-erasures-correct-d61-f17", "k8_62", 61, K8_ALL, 16, ERASURES, CORRECT, erased=tuple(range(1, 18)), offset=8)
    add("k8_62-erasures-report-d61-f3-e6", "k8_62", 61, K8_ALL, 16, ERASURES, REPORT, faulty=6, erased=(0, 12, 25))
    # pss155 (260 rows, k = 100: 25 groups), dimension 250: 3 batches, 50 padding sums the mask job has no entry for
    add("pss155-locate-correct-d250-row1", "pss155", 250, PSS_260, 5, LOCATE, CORRECT, faulty=1, q_mask=TSS_P)
    add("pss155-decode-correct-d250-rows2", "pss155", 250, PSS_260, 5, DECODE, CORRECT, faulty=2, q_mask=TSS_P, offset=8)
    add("pss155-erasures-correct-d250-f1-e1", "pss155", 250, PSS_260, 5, ERASURES, CORRECT, faulty=1, erased=(258,), q_mask=P62)
    # ChaCha: seeds (above), no seed at all, a located seed whose repaired sum is read; None with NULL c and with a begun combiner
    add("k3_62-locate-correct-d769-chacha-noseed", "k3_62", 769, ALL8, 4, LOCATE, CORRECT, faulty=1, masking="chacha", masks="noseed")
    add("k3_62-decode-correct-d8-chacha-rejecting", "k3_62", 8, ALL8, 4, DECODE, CORRECT, faulty=2, masking="chacha", q_mask=cr.Q8, masks="r2_at_0")
    add("k3_62-decode-correct-d766-none-null", "k3_62", 766, ALL8, 4, DECODE, CORRECT, faulty=2, masking="none-null", q_mask=0, masks="none")
    add("k3_62-locate-correct-d764-none-combiner", "k3_62", 764, ALL8, 4, LOCATE, CORRECT, faulty=1, masking="none-combiner", q_mask=0, masks="none",
        offset=8)
    add("k3_62-erasures-correct-d4-none-null", "k3_62", 4, ALL8, 4, ERASURES, CORRECT, erased=(6,), masking="none-null", q_mask=0, masks="none",
        gates="null")
    # q_mask below the sharing modulus, any-int64 rows and masks: masked values at or above q_mask; the corrections are whatever
    # the verdicts on such rows are.  Then sums with faults, so that corrected values are canonicalised
    for end in ENDS:
        add(f"k3_62-{ENDS[end]}-correct-d769-full61-crafted", "k3_62", 769, ALL8, 4, end, CORRECT, erased=(2,) if end == ERASURES else (),
            values="crafted", q_mask=Q61, masks="crafted", offset=8 * (end % 2))
    add("k3_62-locate-correct-d766-full61-row1", "k3_62", 766, ALL8, 4, LOCATE, CORRECT, faulty=1, q_mask=Q61)
    add("k3_62-decode-correct-d766-full61-rows2", "k3_62", 766, ALL8, 4, DECODE, CORRECT, faulty=2, q_mask=Q61, offset=8)
    add("k3_62-erasures-correct-d766-chacha61-f1-e1", "k3_62", 766, ALL8, 4, ERASURES, CORRECT, faulty=1, erased=(4,), masking="chacha", q_mask=Q61,
        masks="seeds")
    # q_mask above the sharing modulus: k3_31 has one surplus row, one check - the erasure end repairs with it, the others report
    add("k3_31-locate-correct-d766-full62-row1", "k3_31", 766, ALL8, 1, LOCATE, CORRECT, faulty=1)
    add("k3_31-erasures-correct-d766-full62-f1", "k3_31", 766, ALL8, 1, ERASURES, CORRECT, erased=(6,), offset=8)
    add("k3_31-erasures-report-d5-full62-crafted", "k3_31", 5, ALL8, 1, ERASURES, REPORT, erased=(0,), values="crafted", masks="crafted")
    # a gate that is shut when the kernel runs: nothing stored, the report written
    add("k3_62-locate-correct-d769-shut-masks", "k3_62", 769, ALL8, 4, LOCATE, CORRECT, faulty=1, word_m=16)
    add("k3_62-decode-correct-d766-shut-results", "k3_62", 766, ALL8, 4, DECODE, CORRECT, faulty=2, word_r=2, offset=8)
    add("k3_62-erasures-correct-d764-shut-equal", "k3_62", 764, ALL8, 4, ERASURES, CORRECT, faulty=1, erased=(5,), gates="equal", word_m=16)
    add("k3_62-decode-correct-d4-none-null-shut-masks", "k3_62", 4, ALL8, 4, DECODE, CORRECT, faulty=1, masking="none-null", q_mask=0, masks="none",
        word_m=1)
    # the pass bits: 16 passes with pass bits 16, shuts with pass bits 0, and 16 | 2 shuts whatever they are
    add("k3_62-erasures-correct-d764-word16-pass16", "k3_62", 764, ALL8, 4, ERASURES, CORRECT, erased=(5,), word_r=16, pass_bits=16)
    add("k3_62-erasures-correct-d764-word16-pass0", "k3_62", 764, ALL8, 4, ERASURES, CORRECT, erased=(5,), word_r=16, pass_bits=0, offset=8)
    add("k3_62-erasures-correct-d764-word18-pass16", "k3_62", 764, ALL8, 4, ERASURES, CORRECT, erased=(5,), word_r=18, pass_bits=16)
    add("k3_62-locate-report-d3-word16-pass16", "k3_62", 3, ALL8, 4, LOCATE, REPORT, faulty=1, word_r=16, pass_bits=16, offset=8)
    parent = len(out)                                              # the table up to here is older than the wide committees

    def more(name, scheme, dim, indices, checks, end, policy, **kw):
        extra = {f: kw.pop(f) for f in ("source", "source_name", "pin", "fill", "bad") if f in kw}
        add(name, scheme, dim, indices, checks, end, policy, **kw)
        out[-1] = out[-1]._replace(**extra)
    # 1. the finish tables' wide committees and steered syndromes, borrowed: the rows their own build() makes, under both policies.
    # Case i of BORROWED is masked by ROTATION[i % 4], its gates (open) take the form GATE_FORMS[i % 3], and the REPORT twin's d_out
    # sits at offset 8 * (i % 2), the CORRECT twin's at the other
    for i, (source, source_name, end) in enumerate(BORROWED):
        for policy, tag in ((REPORT, "report"), (CORRECT, "correct")):
            more(f"{ENDS[end]}-{tag}-from-{source_name}", *_borrowed(source, source_name), end, policy, offset=8 * ((i + policy) % 2),
                 gates=GATE_FORMS[i % 3], **ROTATION[i % 4][1], **_borrowed_fields(source, source_name))
    # 2. sparse faults over five workgroups (1100 batches): clean rows but for the listed batches.  The first bad batch is 300
    # (workgroup 1, lane 44 of its wave), batches 300 and 301 blame one position and 302 another, batch 700 (workgroup 2) holds one
    # error more than the end corrects, workgroups 0 and 3 are clean, the last batch is bad and decoded
    for scheme, dim, indices, checks, hi, many in (("k3_62", 3299, ALL8, 4, 6, (4, 1, 6)), ("k3_wide", 3298, vc.WIDE_300, 16, 257, tuple(range(3, 300, 37)))):
        last = len(indices) - 1
        one = ((300, (2,)), (301, (2,)), (302, (hi,)), (700, (1, last)), (1099, (last,)))
        more(f"{scheme}-locate-correct-d{dim}-sparse", scheme, dim, indices, checks, LOCATE, CORRECT, values="sparse", bad=one, offset=8)
        cap = checks // 2
        some = ((300, many[:cap - 1] + (2,)), (301, (2, 5)), (302, (hi,)), (303, (5, hi)), (700, many[:cap + 1]), (1099, (0, last)))
        for policy, tag in ((CORRECT, "correct"), (REPORT, "report")):
            more(f"{scheme}-decode-{tag}-d{dim}-sparse", scheme, dim, indices, checks, DECODE, policy, values="sparse", bad=some,
                 masking="chacha", masks="seeds", offset=8 * policy)
        gone = (3,) if scheme == "k3_62" else (256,)                      # e' = 1 and 7
        room = (checks - 1) // 2
        few = ((300, (2,)), (301, (2, 258) if room > 1 else (2,)), (302, (hi,)), (700, many[:room + 1]), (1099, (last,)))
        more(f"{scheme}-erasures-correct-d{dim}-sparse", scheme, dim, indices, checks, ERASURES, CORRECT, values="sparse", bad=few, erased=gone,
             q_mask=Q61, masks="crafted", gates="equal")
    # 3. the guard geometry of unmask_store_group.  k8_62 folds 4 + 4: dimension mod 8 = 1 .. 4 leaves the second group of the last
    # batch with have = 0 (the mask base forced to 0) and the first with have = 1, 2, 3, 4; 6 and 7 leave the second with 2 and 3
    # (5 is the older cases').  pss155 with the padding beginning at a group boundary (248), one past it (249) and one before the
    # next (251); one batch of dimension 1 on both
    more("k8_62-locate-correct-d57-row1", "k8_62", 57, K8_ALL, 16, LOCATE, CORRECT, faulty=1, offset=8)
    more("k8_62-decode-correct-d58-rows8", "k8_62", 58, K8_ALL, 16, DECODE, CORRECT, faulty=8)
    more("k8_62-erasures-correct-d59-f3-e6", "k8_62", 59, K8_ALL, 16, ERASURES, CORRECT, faulty=6, erased=(0, 12, 25), offset=8)
    more("k8_62-locate-correct-d60-row1", "k8_62", 60, K8_ALL, 16, LOCATE, CORRECT, faulty=1, q_mask=Q61, masks="crafted")
    more("k8_62-decode-correct-d62-rows8", "k8_62", 62, K8_ALL, 16, DECODE, CORRECT, faulty=8, offset=8)
    more("k8_62-erasures-correct-d63-f16", "k8_62", 63, K8_ALL, 16, ERASURES, CORRECT, erased=tuple(range(1, 17)), masking="chacha", masks="seeds")
    more("pss155-locate-correct-d248-row1", "pss155", 248, PSS_260, 5, LOCATE, CORRECT, faulty=1, q_mask=TSS_P)
    more("pss155-decode-correct-d249-rows2", "pss155", 249, PSS_260, 5, DECODE, CORRECT, faulty=2, q_mask=TSS_P, offset=8)
    more("pss155-erasures-correct-d251-f1-e1", "pss155", 251, PSS_260, 5, ERASURES, CORRECT, faulty=1, erased=(258,), q_mask=P62)
    more("k8_62-decode-correct-d1-rows8", "k8_62", 1, K8_ALL, 16, DECODE, CORRECT, faulty=8, offset=8)
    more("pss155-locate-correct-d1-row1", "pss155", 1, PSS_260, 5, LOCATE, CORRECT, faulty=1, q_mask=TSS_P)
    # 4. deeper mask sums: 40 any-int64 mask rows (3 rows keep the high word of a 128-bit sum within -2 .. 1; what these reach the
    # reach test computes), the smallest masking modulus, and the largest: make_mod takes 2 <= m < 2^62, and Full asks no more of
    # its modulus, so 2^62 - 1 it is
    for end, rows in ((LOCATE, dict(faulty=1)), (DECODE, dict(faulty=2)), (ERASURES, dict(faulty=1, erased=(5,)))):
        more(f"k3_62-{ENDS[end]}-correct-d769-full61-masks40", "k3_62", 769, ALL8, 4, end, CORRECT, q_mask=Q61, masks="crafted40", offset=8 * (end % 2), **rows)
    more("k3_62-decode-correct-d766-full2-crafted", "k3_62", 766, ALL8, 4, DECODE, CORRECT, faulty=2, q_mask=2, masks="crafted")
    more("k3_62-locate-correct-d766-fullmax-row1", "k3_62", 766, ALL8, 4, LOCATE, CORRECT, faulty=1, q_mask=Q_MAX, offset=8)
    # 5. a wide committee behind a gate that is shut when the kernel runs: nothing stored, the whole report - the blame words past
    # position 255 too - written
    for (source, source_name, end), tag, gate in zip(SHUT_WIDE, ("masks", "results", "equal"),
                                                     (dict(word_m=16), dict(word_r=2), dict(gates="equal", word_m=16))):
        more(f"{ENDS[end]}-correct-from-{source_name}-shut-{tag}", *_borrowed(source, source_name), end, CORRECT, offset=8 * (end % 2),
             **gate, **_borrowed_fields(source, source_name))
    return out, parent


Q_MAX = (1 << 62) - 1                                                   # the largest modulus make_mod accepts
GATE_FORMS = ("two", "null", "equal")
# the masking arrangements of the borrowed cases, in rotation
ROTATION = (("Full over P62, random masks", dict(masking="full", q_mask=P62, masks="random")),
            ("Full over Q61, crafted any-int64 masks", dict(masking="full", q_mask=Q61, masks="crafted")),
            ("ChaCha, five seeds, over P62", dict(masking="chacha", q_mask=P62, masks="seeds")),
            ("None, c = NULL", dict(masking="none-null", q_mask=0, masks="none")))
# every case that came with the wide committees and the steered syndromes of the three finish tables
BORROWED = tuple([("reveal_check_cases", c.name, LOCATE) for c in vc.CASES if c.scheme == "k3_wide" or c.fault == "steered"]
                 + [("reveal_decode_cases", n, DECODE) for n in dc.NEW] + [("reveal_erasure_cases", n, ERASURES) for n in ec.NEW])
SHUT_WIDE = (("reveal_check_cases", "k3_wide-c16-d769-row", LOCATE), ("reveal_decode_cases", "k3_wide-c16-d769-rows2", DECODE),
             ("reveal_erasure_cases", "k3_wide-c16-d769-f5-e5-zero", ERASURES))
assert set(SHUT_WIDE) <= set(BORROWED)


def _borrowed(source, source_name):
    """scheme, dim, indices, checks of the source case"""
    c = SOURCES[source].BY_NAME[source_name]
    return c.scheme, c.dim, tuple(c.indices), c.checks


def _borrowed_fields(source, source_name):
    c = SOURCES[source].BY_NAME[source_name]
    return dict(source=source, source_name=source_name, values="borrowed", cap=getattr(c, "cap", 0), pin=c.pin, erased=getattr(c, "erased", ()),
                fill=getattr(c, "fill", "zero"), ok=getattr(c, "ok", "flags"))


CASES, PARENT_CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
NEW = tuple(c.name for c in CASES[PARENT_CASES:])                        # ... and these came with the wide committees
BORROWED_NAMES = tuple(c.name for c in CASES if c.source)

# faults of the unmasking and of the gate; then of the glue around the shared decoder walks, which the 1100-batch cases and the
# guard cases are there for; then of the mask sums' high word
GLUE_FAULTS = ("first_bad_workgroup_local", "first_bad_from_first_lane", "blame_once_per_wave", "second_group_unguarded", "last_element_dropped")
FAULTS = ("correction_after_canonicalisation", "no_canonicalisation", "subtraction_under_sharing_modulus", "padding_stored", "gate_ignored",
          "pass_bits_ignored", "report_suppressed") + GLUE_FAULTS + ("mask_hi_kept_to_4_bits",)
# faults planted in the FINISH models (their GAP_PLANTS), which model() hands on to the source table's model_finish
FINISH_PLANTS = {LOCATE: ("position_mod_256",), DECODE: dc.GAP_PLANTS, ERASURES: ec.GAP_PLANTS}


def has_mask(case):
    return case.masking in ("full", "chacha")


def batches(case):
    return -(-case.dim // rc.SCHEMES[case.scheme][1])


def report_words(case):
    """sda_reconstruct_report_words for the locating end, sda_reconstruct_decode_report_words for the other two"""
    return (4 if case.end == LOCATE else dc.HEAD) + len(case.indices)


def modulus_relation(case):
    p = rc.SCHEMES[case.scheme][0]
    return "none" if not has_mask(case) else "equal" if case.q_mask == p else "below" if case.q_mask < p else "above"


def padding_form(case):
    """how many sums of the last batch are padding"""
    k = rc.SCHEMES[case.scheme][1]
    return batches(case) * k - case.dim


def gate_shut(case, pass_bits=None):
    pass_bits = case.pass_bits if pass_bits is None else pass_bits
    if case.gates == "null":
        return False
    word_m, word_r = (case.word_m | case.word_r,) * 2 if case.gates == "equal" else (case.word_m, case.word_r)
    return word_m != 0 or (word_r & ~pass_bits) != 0


def gate_words(case):
    """the two 32-bit status words as the call finds them (equal: the first alone is used)"""
    if case.gates == "equal":
        return np.array([case.word_m | case.word_r, 0], dtype="<u4")
    return np.array([case.word_m, case.word_r], dtype="<u4")


def ok_words(case):
    """the d_ok array (None: NULL)"""
    if case.end != ERASURES or case.ok == "null":
        return None
    ok = np.ones(len(case.indices), dtype=np.uint32)
    ok[list(case.erased)] = 0
    if case.ok == "ones":
        ok[:] = np.arange(1, len(ok) + 1, dtype=np.uint32) * 0x01010101      # any non-zero word (reveal_erasure_cases.ok_words)
    return ok


Built = collections.namedtuple("Built", "rows mask_rows")
_SPECIAL = uc._SPECIAL


def _special_matrix(rng, shape):
    """three quarters of the values negative: columns whose 128-bit sum is negative (unmask_jobs_cases.build)"""
    special = np.array(_SPECIAL, dtype=np.int64)
    m = special[rng.integers(0, 4, size=shape)]
    mixed = rng.integers(0, 4, size=shape) == 0
    m[mixed] = special[rng.integers(0, special.size, size=int(mixed.sum()))]
    return m


@functools.lru_cache(maxsize=None)
def build(name):
    """rows [positions][batches] int64 for update_dev; mask_rows: Full [3][dim] vectors, ChaCha [seeds][4] seed words, None empty"""
    case = BY_NAME[name]
    p, k, t, n, w2, w3 = rc.SCHEMES[case.scheme]
    rng = np.random.default_rng(zlib.crc32(("unmask-checked/" + name).encode()))
    pos, B = len(case.indices), batches(case)
    if case.values == "borrowed":                                            # the source's rows as they are, its erased rows as it filled them
        rows = SOURCES[case.source].build(case.source_name).rows.view()
        assert rows.shape[0] == pos and rows.shape[1] >= B
    elif case.values == "crafted":
        rows = _special_matrix(rng, (pos, B))
    else:
        x = [pow(w3, i + 1, p) for i in case.indices]
        rows = np.zeros((pos, B), dtype=np.int64)
        for b in range(B):
            g = [int(c) for c in rng.integers(0, p, size=t + k)]
            for i, xi in enumerate(x):
                acc = 0
                for c in reversed(g):
                    acc = (acc * xi + c) % p
                rows[i, b] = (xi - 1) * acc % p
        others = [i for i in range(pos) if i not in case.erased]
        for i in sorted(others[int(j)] for j in rng.permutation(len(others))[:case.faulty]):
            rows[i] = ((rows[i].astype(object) + rng.integers(1, p, size=B, dtype=np.int64).astype(object)) % p).astype(np.int64)
        for b, at in case.bad or ():                                        # sparse: errors in the listed batches only
            assert case.values == "sparse" and not case.faulty and not set(at) & set(case.erased) and len(set(at)) == len(at)
            for i in at:
                rows[i, b] = (int(rows[i, b]) + int(rng.integers(1, p))) % p
    for j in case.erased if case.values != "borrowed" else ():
        rows[j, :] = 0
    if case.masking == "full" and case.masks == "crafted40":
        mask_rows = _special_matrix(rng, (40, case.dim))
        mask_rows[:, 1::2] = ~mask_rows[:, 1::2]                            # odd columns: three quarters of the values positive
    elif case.masking == "full":
        mask_rows = rng.integers(0, case.q_mask, size=(3, case.dim), dtype=np.int64) if case.masks == "random" else _special_matrix(rng, (3, case.dim))
    elif case.masking == "chacha":
        mask_rows = {"seeds": rng.integers(0, 1 << 32, size=(5, 4), dtype=np.int64), "noseed": np.zeros((0, 4), dtype=np.int64)}.get(case.masks)
        if mask_rows is None:
            mask_rows = np.array([cr.SEEDS[case.masks][0]], dtype=np.int64)
    else:
        mask_rows = np.zeros((0, 0), dtype=np.int64)
    rows.setflags(write=False)
    mask_rows.setflags(write=False)
    return Built(rows, mask_rows)


FINISH_MODELS = {LOCATE: vc.model_finish, DECODE: dc.model_finish, ERASURES: ec.model_finish}
_ROOTS = {}
for _c in CASES:
    if _c.source:
        _ROOTS.setdefault((_c.source, _c.source_name, _c.end), _c.name)


def root(name):
    """the first case of the table with this case's rows and end: borrowed twins (the two policies, a shut gate) share one finish"""
    case = BY_NAME[name]
    return _ROOTS[case.source, case.source_name, case.end] if case.source else name


@functools.lru_cache(maxsize=None)
def _finish_padded(name, policy, plant):
    """the finish model over batches * k sums, the last batch's padding included: the first `dim` are what the finish stores"""
    case = BY_NAME[name]
    padded = case._replace(dim=batches(case) * rc.SCHEMES[case.scheme][1])
    return FINISH_MODELS[case.end](padded, build(name).rows, policy, plant=plant)


def finish(name, policy=None, plant=None):
    """the named finish's model on the case's rows (its out, its report ...), under the case's policy or another; plant: a fault of
    FINISH_PLANTS planted in that model"""
    case = BY_NAME[name]
    full = _finish_padded(root(name), case.policy if policy is None else policy, plant)
    return full._replace(out=full.out[:case.dim])


@functools.lru_cache(maxsize=None)
def blamed(name):
    """per batch, the positions the finish blames, ascending (the order of the kernels' slots) - from the finish model's decoded
    errors; the locating model keeps none, so the located position is found again by its rule"""
    case, fin = BY_NAME[name], finish(name)
    if case.end != LOCATE:
        return tuple(tuple(sorted(i for i, _ in fin.errors[b])) if isinstance(v, int) and v > 0 else () for b, v in enumerate(fin.verdicts))
    T = vc.tables(case.scheme, case.indices, case.checks)
    rows, out = build(name).rows, []
    for b, v in enumerate(fin.verdicts):
        at = ()
        if v == "located":
            sh = [int(rows[i][b]) % T.p for i in range(len(case.indices))]
            S = [sum(h * s for h, s in zip(T.H[d], sh)) % T.p for d in range(case.checks)]
            at = tuple(i for i, x in enumerate(T.x) if all(S[d + 1] == x * S[d] % T.p for d in range(case.checks - 1)))
            assert len(at) == 1
        out.append(at)
    return tuple(out)


def mask_high_words(name):
    """the high words of the mask job's 128-bit sums"""
    return [s >> 64 for s in mask_sums(name)]


@functools.lru_cache(maxsize=None)
def mask_sums(name):
    """the mask job's `dim` exact sums (None masking: none)"""
    case, b = BY_NAME[name], build(name)
    if case.masking == "full":
        return tuple(sum(int(r[i]) for r in b.mask_rows) for i in range(case.dim))
    if case.masking == "chacha":
        per_seed = [uc.chacha_masks([int(w) for w in s], case.q_mask, case.dim) for s in b.mask_rows]
        return tuple(sum(m[i] for m in per_seed) for i in range(case.dim))
    return ()


Model = collections.namedtuple("Model", "buffer report_buffer out report shut")


def _last_group(case):
    """(e0, n, have) of the group of four that holds the output's last element"""
    k = rc.SCHEMES[case.scheme][1]
    b, s = divmod(case.dim - 1, k)
    s0 = s // 4 * 4
    e0, n = b * k + s0, min(4, k - s0)
    return e0, n, min(n, case.dim - e0)


def group_haves(case):
    """`have` of every group of the LAST batch (every other batch has full groups): what unmask_group_have returns there"""
    k = rc.SCHEMES[case.scheme][1]
    e = (batches(case) - 1) * k
    return tuple(max(0, min(min(4, k - s0), case.dim - (e + s0))) for s0 in range(0, k, 4))


@functools.lru_cache(maxsize=None)
def model(name, faults=frozenset()):
    """What the call leaves in two sentinel-filled buffers - offset / 8 + dim + TAIL words whose output starts at word offset / 8,
    and report_words + TAIL words - in Python integers.  `faults` plants one of FAULTS, or one of the end's FINISH_PLANTS in the
    finish model underneath."""
    case = BY_NAME[name]
    p, k = rc.SCHEMES[case.scheme][:2]
    qm = case.q_mask
    plant = next((f for f in faults if f in FINISH_PLANTS[case.end]), None)
    fin = finish(name, plant=plant)
    v = [int(x) for x in fin.out]
    if "padding_stored" in faults:                                          # the lanes' padding secrets, unmasked with no mask
        v = [int(x) for x in _finish_padded(root(name), case.policy, None).out]
    if has_mask(case):
        sums = mask_sums(name)
        if "mask_hi_kept_to_4_bits" in faults:                              # the sum's high word sign-extended from its low four bits
            sums = [(((s >> 64) + 8) % 16 - 8 << 64) + (s & (1 << 64) - 1) for s in sums]
        mask = [s % qm for s in sums] + [0] * (len(v) - case.dim)
        if "correction_after_canonicalisation" in faults:                   # the correction (a residue of p) taken off under q_mask
            plain = [int(x) for x in finish(name, REPORT).out]
            delta = [(a - b) % p for a, b in zip(plain, v)]
            x = [(a % qm - d) % qm for a, d in zip(plain, delta)] + v[case.dim:]
            out = [(a - y) % qm for a, y in zip(x, mask)]
        elif "no_canonicalisation" in faults:                               # submod on the operand as it came
            out = [(a - y if a >= y else a + qm - y) for a, y in zip(v, mask)]
        elif "subtraction_under_sharing_modulus" in faults:
            out = [(a - y) % p for a, y in zip(v, mask)]
        else:
            out = [(a % qm - y) % qm for a, y in zip(v, mask)]
    else:
        mask = [0] * len(v)
        out = list(v)
    shut = gate_shut(case, 0 if "pass_bits_ignored" in faults else None)
    head = case.offset // 8
    buf = [SENTINEL] * (head + case.dim + TAIL)
    if not shut or "gate_ignored" in faults:
        for i in range(min(len(out), case.dim + TAIL)):
            buf[head + i] = out[i]
        if "second_group_unguarded" in faults and k == 8 and group_haves(case)[1] == 0:
            # the second group of the last batch - all padding: folded, never corrected - is unmasked with the mask entries of the
            # output's FIRST elements (the base forced to 0) and stored where it would lie: in the tail words behind the output
            e0 = (batches(case) - 1) * k + 4
            folded = [int(x) for x in _finish_padded(root(name), REPORT, None).out]
            for j in range(4):
                y = mask[j] if j < case.dim else 0
                buf[head + e0 + j] = (folded[e0 + j] % qm - y) % qm if has_mask(case) else folded[e0 + j]
        if "last_element_dropped" in faults:                                # `have` one short in a partial group: the last element stays
            e0, n, have = _last_group(case)
            if have < n:
                buf[head + case.dim - 1] = SENTINEL
    words = [int(w) for w in fin.report]
    assert len(words) == report_words(case)
    firsts = (3,) if case.end == LOCATE else (3, 4)                        # the first bad batch; the first undecoded one
    for w in firsts:
        if words[w] != vc.NONE64 and "first_bad_workgroup_local" in faults:      # taken relative to its workgroup of 256 lanes
            words[w] %= 256
        if words[w] != vc.NONE64 and "first_bad_from_first_lane" in faults:      # the wave's first batch, not its first bad one
            words[w] -= words[w] % 64
    if "blame_once_per_wave" in faults:                                     # 1, not the lane count, per position a wave blames in a slot
        at = report_words(case) - len(case.indices)
        seen = {(b // 64, j, i) for b, pos in enumerate(blamed(name)) for j, i in enumerate(pos)}
        words[at:] = [sum(1 for _, _, i in seen if i == q) for q in range(len(case.indices))]
    rep = (words if not (shut and "report_suppressed" in faults) else [SENTINEL] * len(words)) + [SENTINEL] * TAIL
    return Model(tuple(buf), tuple(rep), tuple(out[:case.dim]), tuple(words), shut)


def want(name):
    """the expected output buffer as int64 and report buffer as uint64"""
    m = model(name)
    return np.array(m.buffer, dtype=np.int64), np.array(m.report_buffer, dtype=np.uint64)
