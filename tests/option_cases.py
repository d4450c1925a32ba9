"""The public options of libzkmi355x (the PUBLIC rows of csrc/zk_options.h) and how the suite holds each of them to the oracle -- TEST INFRASTRUCTURE ONLY.

include/zkmi355x.h (zk_set_option) promises that no public knob changes a result.  CASES has one row per public name: the values to exercise (every
branch its parse site tells apart), where the library reads it, and the companion settings a value needs to reach its branch.  tests/test_option_cases.py
(CPU) keeps the table equal to the PUBLIC rows of csrc/zk_options.h (option_table below reads them) and the `read` column true to each row's kind;
tests/test_gpu_options.py (GPU) runs it.  ROUTES, further down, has one row per way to make a handle: tests/test_gpu_options_routes.py (GPU) runs CASES
through every one of them.

read:    from the row's kind in csrc/zk_options.h
  "cached" -- a CACHED row: fixed at its first read, so only a fresh process reaches another value (CACHED_GROUPS below, one child process per group).
  "setup"  -- a LIVE row read when a key is uploaded, a slot's workspaces are allocated or a key is derived: set before the upload, live in one process.
  "call"   -- read per call: a FORM row (under ZK_TEST_FORMS=1, which tests/conftest.py sets), or a LIVE row on a per-call path.
size:    "small" -- Groth16 at 2^12, Pinocchio at n = 1000;  "ba" -- both at 2^14, where the automatic batch-affine rounds start.
multi:   also run on the device lists [0, 0] and [0, 0, 0] (the one card listed several times, as tests/test_gpu_multidevice.py does).
special: "msm_api" -- reached through zk_msm_g1 / zk_msm_g2 against the oracle's naive fold instead of through a proof.
"""
import os
import re
from collections import namedtuple

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "zukelang_amd", "csrc")
OPTIONS_UNIT = "zk_options.h"
# every way a unit of the library touches an option (csrc/zk_options.h): any opt_*( call, whatever its argument, or one of the three named readers.
# Groups: the opt_* function, the row's id where the argument is a literal one, the named reader.
OPTION_READ = re.compile(r"\b(?:(opt_\w+)\s*\(\s*(?:OPT_([A-Z0-9_]+))?|(key_subgroup_check|trace_on|forms_live)\s*\()")
OptionRow = namedtuple("OptionRow", "id name kind visibility")


def option_table():
    """the rows of csrc/zk_options.h, in order"""
    text = open(os.path.join(CSRC, OPTIONS_UNIT)).read()
    rows = [OptionRow(*m) for m in re.findall(r'^\s*ZK_OPTION\(\s*(\w+)\s*,\s*"(ZK_[A-Z0-9_]+)"\s*,\s*(\w+)\s*,\s*(\w+)\s*\)', text, flags=re.M)]
    assert rows and all(r.name == "ZK_" + r.id and r.kind in ("CACHED", "LIVE", "FORM") and r.visibility in ("PUBLIC", "INTERNAL", "ENV_ONLY") for r in rows)
    assert len({r.name for r in rows}) == len(rows), "a name listed twice in zk_options.h"
    return rows


def public_options():
    return [r.name for r in option_table() if r.visibility == "PUBLIC"]


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


# ---- the routes to a handle.  CASES above says WHICH settings to run; ROUTES says THROUGH WHAT.  tests/test_gpu_options.py is the first route
# (PROVE_ROUTE: uncompressed upload, derivation, prove / prove_async); tests/test_gpu_options_routes.py runs every live setting, every cached group
# and the named interactions through each row below.  What is expected never comes from the library at its default options: proofs from the trapdoor
# oracles, sums from the oracle's naive fold, masks from the integer models, key bytes from the host keygen (itself held to the oracle's setup).
#
# entry:   the C entry points of include/zkmi355x.h the row ANSWERS FOR: each name stands in one row only, so a deleted row leaves its names
#          uncovered (tests/test_option_cases.py: every key, proving, pool and resident-MSM call of the header is in a row, in PROVE_ROUTE or in
#          EXEMPT).  Every proving route also runs zk_*_prove and zk_*_prove_many_compressed on its handle
# with_ba: companions added to the rows of size "ba" -- the route's key has a size of its own, and the automatic batch-affine rounds need a mean of
#          8 entries per bucket (msm.hip: ba_rounds_for); test_option_cases.py does the arithmetic
# multi:   what a row with multi=True asks of the route on the device list [0, 0]: "proofs" -- the single-device bytes; "bytes" -- zk_*_keygen
#          gives no handle on a device list (ZK_ERR_ARG), the key bytes are still keygen's; None -- not run (key checks refuse such handles, resident
#          bases live on the list's first device: both tested where those calls are)
Route = namedtuple("Route", "entry protocol with_ba multi")

PROVE_ROUTE = ("zk_groth16_pk_upload", "zk_groth16_prove", "zk_groth16_prove_async", "zk_groth16_prove_wait",
               "zk_pinocchio_pk_upload", "zk_pinocchio_prove", "zk_pinocchio_prove_async", "zk_pinocchio_prove_wait")

ROUTES = {
    "g16_wire": Route(("zk_groth16_pk_upload_compressed", "zk_groth16_prove_many_compressed"), "groth16", {}, "proofs"),
    "g16_generated": Route(("zk_groth16_keygen", "zk_groth16_pool_points"), "groth16", {}, "bytes"),
    # the pools of a derived handle out in wire form, in again as a Lagrange-form key (what a key cache does)
    "g16_cached_lagrange": Route(("zk_groth16_pool_points_compressed",), "groth16", {}, None),
    # the n1025 circuit of tests/test_gpu_key_check.py (KEY_CHECK_POOLS); the Lagrange-form keys go up through zk_groth16_pk_upload_lagrange
    "g16_key_check": Route(("zk_groth16_key_check", "zk_groth16_key_check_lagrange", "zk_groth16_pk_upload_lagrange"), "groth16", {"ZK_MSM_WINDOW": "8"}, None),
    "pin_wire": Route(("zk_pinocchio_pk_upload_compressed", "zk_pinocchio_pool_points_compressed", "zk_pinocchio_prove_many_compressed"), "pinocchio", {}, "proofs"),
    "pin_generated": Route(("zk_pinocchio_keygen",), "pinocchio", {}, "bytes"),
    "pin_lagrange": Route(("zk_pinocchio_pk_upload_lagrange", "zk_pinocchio_pool_points"), "pinocchio", {}, None),
    "resident": Route(("zk_bases_upload", "zk_bases_upload_compressed", "zk_msm_resident", "zk_msm_resident_many"), "msm", {}, None),
}

# which entry points of the header the table must account for, and the ones it leaves out on purpose
ROUTED_WORDS = ("prove", "pk_upload", "keygen", "key_check", "msm_resident", "bases_upload", "pool_points")
EXEMPT = {
    "zk_groth16_pk_upload_sharded": "a device list builds its shards through the same code: the multi rows of both option modules",
    "zk_groth16_prove_partial": "a shard's half of a proof: what a multi-device handle runs per device (multi rows)",
    "zk_groth16_prove_partial_async": "as zk_groth16_prove_partial (multi rows)",
    "zk_groth16_prove_partial_wait": "as zk_groth16_prove_partial (multi rows)",
    "zk_groth16_prove_partial_wait_device": "as zk_groth16_prove_partial, the sums left on the device (tests/test_gpu_groth16.py)",
}
# the verifiers have no row because they read no option: test_option_cases.py holds that to their sources
VERIFIER_SOURCES = ("pairing_dev.hip", "verify_resident.hip", "pairing_host.hip")

# the pools of the key-check route's key, per form: what ba_rounds_for sees
KEY_CHECK_POOLS = {"tau_powers": (3089, 1029), "lagrange": (3087, 1027)}

# the named interactions of tests/test_gpu_options_routes.py: a handle meets setting A, then setting B, in both directions
FLIPS = {
    "ba_rounds": {"ZK_MSM_BA_ROUNDS": "2"},
    "window5": {"ZK_MSM_WINDOW": "5"},
    "window17": {"ZK_MSM_WINDOW": "17"},
    "two_level16": {"ZK_MSM_WINDOW": "16", "ZK_SORT_TWO_LEVEL_MIN": "10"},
}


def route_settings(route, c, settings):
    """the settings of a live run as the route runs them: its companions for the row's size, never over what the row itself sets"""
    extra = ROUTES[route].with_ba if c.size == "ba" else {}
    return dict(extra, **settings)


def live_runs():
    """(id, settings) for every value of every row a proof in this process can reach: not cached, not special."""
    out = []
    for name, c in CASES.items():
        if c.read == "cached" or c.special:
            continue
        for v in c.values:
            out.append(("%s=%s" % (name, v), c, dict(c.with_, **{name: v})))
    return out
