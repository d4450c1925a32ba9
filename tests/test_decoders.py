"""The host decoders -- zk_g1/g2_decompress and the uncompressed decoder behind zk_pairing_product (csrc/pairing_host.hip) -- against the decoder
oracle of oracle/pyref.py (written from the ZCash serialization rules in plain big integers) over the encoding matrix of tests/encoding_cases.py:
valid points, flag bits that contradict the string, coordinates out of range, abscissae off the curve and points outside the subgroup.  And the
wire readers on records whose point strings have the wrong length or are malformed identities.  No GPU, and nothing here calls the library's
ENCODERS: the host-only sanitizer build (tests/test_sanitizers.py) runs this file too, so a decoder that reads past a Python buffer is a red test."""
import ctypes as C
import os

import pytest

import encoding_cases as E
from oracle import pyref as P
from zukelang_amd import _lib, wire

ZK_ERR_ARG, ZK_ERR_NOT_ON_CURVE = -1, -2
WANT = {P.OK: 0, P.BAD_ENCODING: ZK_ERR_ARG, P.NOT_ON_CURVE: ZK_ERR_NOT_ON_CURVE, P.NOT_IN_SUBGROUP: ZK_ERR_NOT_ON_CURVE}
G1_INF, G2_INF = bytes([0x40]) + bytes(95), bytes([0x40]) + bytes(191)


def host_decode(group, compressed, data):
    """-> (status, uncompressed bytes).  Uncompressed strings go through zk_pairing_product next to the other group's identity: both points are decoded
    and checked, and an accepted point IS its canonical string."""
    L = _lib.lib()
    if compressed:
        out = C.create_string_buffer(96 * group)
        rc = (L.zk_g1_decompress if group == 1 else L.zk_g2_decompress)(bytes(data), out)
        return rc, out.raw
    gt = C.create_string_buffer(576)
    g1, g2 = (bytes(data), G2_INF) if group == 1 else (G1_INF, bytes(data))
    return L.zk_pairing_product(g1, g2, C.c_size_t(1), gt), bytes(data)


@pytest.mark.parametrize("compressed", [True, False], ids=["compressed", "uncompressed"])
@pytest.mark.parametrize("group", [1, 2], ids=["G1", "G2"])
def test_host_decoders_agree_with_the_oracle_on_the_encoding_matrix(group, compressed):
    rows = E.matrix(group, compressed)
    kinds = {k: 0 for k in E.KINDS}
    verdicts = {v: 0 for v in WANT}
    wrong = []
    for case, verdict, point in rows:
        kinds[case.kind] += 1
        verdicts[verdict] += 1
        rc, out = host_decode(group, compressed, case.data)
        if rc != WANT[verdict] or (verdict == P.OK and out != point):
            wrong.append((case.kind, case.label, case.data.hex(), "oracle: %s" % verdict, "library: %d" % rc))
    assert all(kinds.values()) and all(verdicts.values()), (kinds, verdicts)          # every class of the matrix is populated: nothing is skipped
    assert not wrong, "%d of %d strings decoded differently: %r" % (len(wrong), len(rows), wrong[:8])


def test_the_matrix_holds_the_named_malformed_identities():
    """E0 00..00, C0 00..01, C1 00..00 (compressed) and 40 00..01, 60 00..00 (uncompressed): refused by the oracle, whatever else the matrix holds."""
    for group in (1, 2):
        comp = {c.data for c in E.cases(group, True)}
        unc = {c.data for c in E.cases(group, False)}
        for first, last in ((0xE0, 0), (0xC0, 1), (0xC1, 0)):
            s = bytes([first]) + bytes(48 * group - 2) + bytes([last])
            assert s in comp and E.oracle_verdict(group, True, s)[0] == P.BAD_ENCODING
        for first, last in ((0x40, 1), (0x60, 0)):
            s = bytes([first]) + bytes(96 * group - 2) + bytes([last])
            assert s in unc and E.oracle_verdict(group, False, s)[0] == P.BAD_ENCODING


# ---------------------------------------------------------------- the wire readers on the golden JSON with one point string replaced
def _golden_records():
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    pkey_js, proof_js = (bytes.fromhex(line) for line in open(os.path.join(here, "readme_groth16_wire.hex")).read().split())
    return [(wire.groth16_pkey_of_json, pkey_js), (wire.groth16_proof_of_json, proof_js)]


def test_readers_refuse_wrong_lengths_and_malformed_identities_in_the_golden_records():
    for reader, record in _golden_records():
        assert E.check_reader_refuses_bad_point_strings(wire, reader, record) >= 2 * len(E.bad_point_strings(1))


def test_one_point_readers_check_the_length_before_the_library_reads():
    good1, good2 = P.g1_compress(P.G1), P.g2_compress(P.G2)
    for fn, good, size in ((wire.g1_of_json, good1, 48), (wire.g2_of_json, good2, 96)):
        assert len(fn(good)) == 2 * size
        lengths = sorted((set(E.WRONG_LENGTHS) | {11, size - 1, size + 1, size + 4}) - {size})
        for n in lengths:
            with pytest.raises(ValueError) as info:
                fn((good * 3)[:n])
            assert E.message_class(info.value) == "length", (n, str(info.value))
