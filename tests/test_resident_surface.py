"""The surface of the resident MSM bases without a GPU: the five C prototypes and their EXPORTS entries, the Python surface of curve.py, the
OCaml seam's physical memoisation (bls12_381_mi355x.ml), and the option table (no new public option name came with the feature)."""
import inspect
import os
import re

import option_cases
from zukelang_amd import _lib, curve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "zkmi355x.h")).read()
SEAM = open(os.path.join(ROOT, "ocaml", "bls12_381_mi355x.ml")).read()

PROTOS = {
    "zk_bases_upload": "int zk_bases_upload(int group, const uint8_t* points, size_t n, uint64_t* handle);",
    "zk_bases_info": "int zk_bases_info(uint64_t handle, int* group, uint64_t* n, uint64_t* short_max);",
    "zk_bases_free": "int zk_bases_free(uint64_t handle);",
    "zk_msm_resident": "int zk_msm_resident(uint64_t handle, const uint8_t* scalars, size_t nscalars, uint8_t* out);",
    "zk_msm_resident_many": "int zk_msm_resident_many(uint64_t handle, const uint8_t* scalars, const uint64_t* lens, uint32_t count, uint8_t* out);",
}


def test_resident_prototypes_and_exports():
    for name, proto in PROTOS.items():
        assert proto in HEADER, name
        assert name in _lib.EXPORTS, name
    lib = _lib.lib()
    assert all(hasattr(lib, n) for n in PROTOS)


def test_resident_python_surface():
    for G in (curve.G1, curve.G2):
        assert callable(G.resident)
        assert list(inspect.signature(G.resident).parameters) == ["points"]
    R = curve.ResidentBases
    for m in ("apply_powers", "apply_powers_many", "close", "__enter__", "__exit__", "__del__"):
        assert callable(getattr(R, m)), m
    assert list(inspect.signature(curve.sum_apply_powers).parameters) == ["G", "ti", "ps", "w"]
    # the per-call entry points stay as they were
    assert list(inspect.signature(curve.G1.apply_powers).parameters) == ["cs", "xis", "window_bits"]
    assert list(inspect.signature(curve.G1.dot).parameters) == ["m", "c", "window_bits"]


def _code(src):
    out, depth, i = [], 0, 0
    while i < len(src):
        if src.startswith("(*", i):
            depth += 1; i += 2
        elif src.startswith("*)", i) and depth:
            depth -= 1; i += 2
        else:
            if not depth:
                out.append(src[i])
            i += 1
    return "".join(out)


def test_ocaml_seam_memoises_physically_and_calls_the_resident_product():
    code = _code(SEAM)
    assert "zk_msm_resident" in code
    tables = re.findall(r"Ephemeron\.K1\.Make\s*\(struct(.*?)end\)", code, flags=re.S)
    assert len(tables) == 2, "one table keyed on the xis list, one on the key map"
    for t in tables:
        assert re.search(r"let\s+equal\s*=\s*\(\s*==\s*\)", t), "keys compare physically"
        assert "List.length" not in t, "an O(n) hash"
        assert "Hashtbl.hash" in t
    assert re.search(r"type nonrec t = t list", code) and re.search(r"type nonrec t = t Var\.Map\.t", code)
    # dot's table is keyed on the map m, not on the fresh list Var.Map.bindings builds
    dot = code[code.index("let dot"):]
    assert re.search(r"By_map\.find_opt by_map\)\s*~replace:\(By_map\.replace by_map\)\s*m\b", dot)


def test_no_new_public_option():
    names = option_cases.public_options()
    assert len(names) == 28
    assert not any("RESIDENT" in n or "SHORT" in n for n in names)
    src = open(os.path.join(ROOT, "zukelang_amd", "csrc", "msm_resident.hip")).read()
    assert "getenv" not in src
    assert [m.group(0) for m in option_cases.OPTION_READ.finditer(src)] == ["key_subgroup_check("]
