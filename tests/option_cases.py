"""The public options of libzkmi355x (csrc/zk_api.hip: PUBLIC_OPTIONS) and how the suite holds each of them to the oracle -- TEST INFRASTRUCTURE ONLY.

include/zkmi355x.h (zk_set_option) promises that no public knob changes a result.  CASES has one row per public name: the values to exercise (every
branch its parse site tells apart), where the library reads it, and the companion settings a value needs to reach its branch.  tests/test_option_cases.py
(CPU) keeps the table equal to PUBLIC_OPTIONS and the `read` column equal to the read sites; tests/test_gpu_options.py (GPU) runs it.

read:
  "cached" -- a function-local static (ZK_ENV, or `static const ... = ::zk::opt(...)`): fixed at first use, so only a fresh process reaches another value
              (CACHED_GROUPS below, one child process per group).
  "setup"  -- read when a key is uploaded, a slot's workspaces are allocated or a key is derived: set before the upload, live in one process.
  "call"   -- read per call (ZK_FORM_ENV under ZK_TEST_FORMS=1, which tests/conftest.py sets, or a plain ::zk::opt on a per-call path).
size:    "small" -- Groth16 at 2^12, Pinocchio at n = 1000;  "ba" -- both at 2^14, where the automatic batch-affine rounds start.
multi:   also run on the device lists [0, 0] and [0, 0, 0] (the one card listed several times, as tests/test_gpu_multidevice.py does).
special: "msm_api" -- reached through zk_msm_g1 / zk_msm_g2 against the oracle's naive fold instead of through a proof.
"""
from collections import namedtuple

Case = namedtuple("Case", "values read with_ size multi special")


def case(values, read, with_=None, size="small", multi=False, special=None):
    return Case(tuple(str(v) for v in values), read, dict(with_ or {}), size, multi, special)


# companions: the reduction forms differ only in a window above 16 bits (digit sums in the wide form), the sort forms only where there are enough buckets
_WIDE = {"ZK_MSM_WINDOW": "19"}
_TWO_LEVEL = {"ZK_MSM_WINDOW": "16", "ZK_SORT_TWO_LEVEL_MIN": "10"}

CASES = {
    # 3, 5, 15, 17 divide 255: folded digits (msm.cuh: msm_fold), one window fewer; 2 and 22 are the ends of the legal range
    "ZK_MSM_WINDOW": case([2, 3, 5, 15, 17, 22], "setup", multi=True),
    # 0: no [r] P = O test at upload and no folded windows; both at a fold width
    "ZK_KEY_SUBGROUP_CHECK": case([0, 1], "setup", {"ZK_MSM_WINDOW": "5"}, multi=True),
    # groth16.hip: atoi >= 3 -> three streams in every slot, otherwise one; ZK_SERIAL_STREAMS set -> one stream even for slot 0 (Pinocchio: no fork)
    "ZK_SLOT_STREAMS": case([1, 3], "cached"),
    "ZK_SERIAL_STREAMS": case([1], "cached"),
    # each slot's Groth16 proof captured into a hipGraph and replayed; Pinocchio must ignore it
    "ZK_GRAPH": case([0, 1], "call"),
    # accumulate chunking (msm.hip: msm_workspace_alloc): a one-entry floor, and a floor above the 64 from which the whole-rounds rule runs;
    # a thread target far below the work (long chunks) and far above it (the floor decides)
    "ZK_MSM_CHUNK_MIN": case([1, 64], "cached"),
    "ZK_MSM_TARGET_THREADS": case([4096, 1 << 24], "cached"),
    # 0 at 2^16 buckets (window 17, folded): the global-atomic sort instead of two levels
    "ZK_SORT_TWO_LEVEL": case([0, 1], "setup", {"ZK_MSM_WINDOW": "17", "ZK_SORT_TWO_LEVEL_MIN": "10"}),
    "ZK_SORT_TWO_LEVEL_MIN": case([10], "setup", {"ZK_MSM_WINDOW": "16"}),
    # workgroups of the single-level LDS sort: 1 takes it at every size, 64 sends small pools to the global atomics
    "ZK_SORT_MIN_WGS": case([1, 64], "cached"),
    "ZK_SORT_SCALAR_MAJOR": case([0], "cached"),
    "ZK_SORT_FINE_STAGED": case([0, 1], "call", _TWO_LEVEL),
    "ZK_SORT_COARSE_STAGED": case([0, 1], "call", _TWO_LEVEL),
    "ZK_TAIL_SLOTS": case([0, 1], "call", _WIDE),
    "ZK_TAIL_FIXUP_SLOTS": case([0, 1], "call", _WIDE),
    "ZK_FIXUP_BY_CHUNK": case([0, 1], "call", _WIDE),
    "ZK_DS_WIDE_GROUP": case([16, 32, 64], "call", dict(_WIDE, ZK_TAIL_SLOTS="0")),
    "ZK_RED_WAVES": case([1, 2], "call", dict(_WIDE, ZK_TAIL_SLOTS="0")),
    "ZK_ACC_G1_GLDS": case([0, 1], "call"),
    "ZK_ACC_G1_MMADD": case([0, 1], "call"),
    "ZK_ACC_G2_INLINE": case([0, 1], "call"),
    # bit 0: G1, bit 1: G2 -- automatic rounds (no ZK_MSM_BA_ROUNDS), which need a mean of 8 entries per bucket: 2^14 points
    "ZK_MSM_BA_CURVES": case([1, 2, 3], "setup", size="ba", multi=True),
    "ZK_MSM_BA_ROUNDS": case([0, 1, 2, 6], "setup", size="ba", multi=True),
    "ZK_MSM_API_PRECOMP": case([1], "call", special="msm_api"),
    "ZK_DERIVE_SIDE_BY_SIDE": case([0, 1], "setup"),
    "ZK_FR_RNS": case([0, 1], "call"),
    # Pinocchio's own switches; Groth16 must ignore them
    "ZK_PIN_SHARED_SORT": case([0, 1], "setup"),
    "ZK_PIN_COMPACT_H": case([0, 1], "setup", multi=True),
}

# The cached knobs, in at most three child processes: every value of every "cached" row appears in one group.  ZK_SERIAL_STREAMS overrides
# ZK_SLOT_STREAMS, so it has a process of its own.
CACHED_GROUPS = [
    {"ZK_SLOT_STREAMS": "3", "ZK_MSM_TARGET_THREADS": str(1 << 24), "ZK_MSM_CHUNK_MIN": "1", "ZK_SORT_MIN_WGS": "1", "ZK_SORT_SCALAR_MAJOR": "0"},
    {"ZK_SLOT_STREAMS": "1", "ZK_MSM_TARGET_THREADS": "4096", "ZK_MSM_CHUNK_MIN": "64", "ZK_SORT_MIN_WGS": "64"},
    {"ZK_SERIAL_STREAMS": "1", "ZK_SORT_SCALAR_MAJOR": "0"},
]


def live_runs():
    """(id, settings) for every value of every row a proof in this process can reach: not cached, not special."""
    out = []
    for name, c in CASES.items():
        if c.read == "cached" or c.special:
            continue
        for v in c.values:
            out.append(("%s=%s" % (name, v), c, dict(c.with_, **{name: v})))
    return out
