"""The encoding matrix of the decoder tests: byte strings no honest encoder wrote next to the ones it does write, per group (1 = G1, 2 = G2) and
per form (compressed, uncompressed), built with oracle/pyref.py alone -- nothing of the product is called here, so the host-only sanitizer build
of the library (which has the decoders and not the encoders) runs the same matrix.

cases(group, compressed) -> [Case(kind, label, data)], kind in KINDS.  What each string SHOULD decode to is not stated here: that is the verdict of
pyref.g1/g2_decompress / g1/g2_decode, which the tests compare the product with."""
import collections

from oracle import pyref as P

Case = collections.namedtuple("Case", "kind label data")
KINDS = ("valid", "flags", "range", "curve")
SEEDED = 64


def _size(group, compressed):
    return (48 if compressed else 96) * group


def _compress(group, pt):
    return (P.g1_compress if group == 1 else P.g2_compress)(pt)


def _to_bytes(group, pt):
    return (P.g1_to_bytes if group == 1 else P.g2_to_bytes)(pt)


def _encode(group, compressed, pt):
    return _compress(group, pt) if compressed else _to_bytes(group, pt)


def _be(v):
    return int(v).to_bytes(48, "big")


_VALID = {}


def valid_points(group):
    """(k, k G) for k in {1, 2, 3, r-1, r-2} and SEEDED seeded scalars, each with its negative: both signs of y."""
    if group not in _VALID:
        st = P.fr_stream(0xE7C0DE00 + group)
        ks = [1, 2, 3, P.R - 1, P.R - 2] + [next(st) for _ in range(SEEDED)]
        gen = P.G1 if group == 1 else P.G2
        pts = []
        for k in ks:
            pt = P.pt_mul_jac(gen, k)
            pts += [pt, P.pt_neg(pt)]
        _VALID[group] = pts
    return _VALID[group]


def malformed_infinities(group, compressed):
    """Infinity bit set and something else set too: the sign bit, a low flag-byte bit, one non-zero byte in the first / a middle / the last position."""
    size = _size(group, compressed)
    c = 0x80 if compressed else 0
    inf = bytearray([c | 0x40]) + bytearray(size - 1)
    out = [("infinity with the sign bit", bytes([c | 0x60]) + bytes(size - 1)),
           ("infinity with a low bit of the flag byte", bytes([c | 0x41]) + bytes(size - 1))]
    for where, pos in (("first", 1), ("middle", size // 2), ("last", size - 1)):
        b = bytearray(inf)
        b[pos] = 1
        out.append(("infinity with a non-zero byte in the %s position" % where, bytes(b)))
    return out


def cases(group, compressed):
    size = _size(group, compressed)
    gen = P.G1 if group == 1 else P.G2
    out = []
    add = lambda kind, label, data: out.append(Case(kind, label, bytes(data)))

    # ---- valid
    add("valid", "identity", _encode(group, compressed, None))
    for i, pt in enumerate(valid_points(group)):
        add("valid", "multiple of the generator #%d" % i, _encode(group, compressed, pt))

    # ---- flags
    good = bytearray(_encode(group, compressed, P.pt_mul_jac(gen, 5)))
    flip = bytearray(good)
    flip[0] ^= 0x80
    add("flags", "compression bit missing" if compressed else "compression bit on an uncompressed string", flip)
    other = bytearray(_encode(group, not compressed, P.pt_mul_jac(gen, 5)))          # the other form's string, cut or padded to this form's size
    add("flags", "the other form's string at this size", (other + bytearray(size))[:size])
    add("flags", "the other form's identity at this size", bytes([0x40 if compressed else 0xC0]) + bytes(size - 1))
    for label, data in malformed_infinities(group, compressed):
        add("flags", label, data)
    if not compressed:
        for i, pt in enumerate(valid_points(group)[:4]):
            b = bytearray(_to_bytes(group, pt))
            b[0] |= 0x20
            add("flags", "sign bit on an uncompressed string #%d" % i, b)

    # ---- range: one coordinate out of range alone, the others taken from the generator
    flag = 0x80 if compressed else 0
    coords = [gen[0].a, gen[1].a] if group == 1 else [gen[0].b, gen[0].a, gen[1].b, gen[1].a]          # the wire order: x | y, x1 | x0 | y1 | y0
    ncoord = size // 48
    for which in range(ncoord):
        for name, v in (("p", P.P), ("p - 1", P.P - 1), ("2^381 - 1", (1 << 381) - 1)):
            for sign in ((0, 0x20) if compressed else (0,)):
                cs = [_be(coords[i]) for i in range(ncoord)]
                cs[which] = _be(v)
                b = bytearray(b"".join(cs))
                b[0] |= flag | sign
                add("range", "coordinate %d = %s, sign bit %#x" % (which, name, sign), b)
    add("range", "all ones", b"\xff" * size)

    # ---- curve / subgroup: small abscissae.  Compressed: both sign bits.  Uncompressed: both roots when x^3 + b is a square, else y = 1 and p - 1.
    if group == 1:
        xs = [(x, None) for x in range(1, 60)]
    else:
        xs = [(x, 0) for x in range(1, 60)] + [(k, 0) for k in range(1, 40)] + [(0, k) for k in range(1, 40)]
        xs = list(dict.fromkeys(xs)) + [(k, k) for k in range(1, 25)]
    for x0, x1 in xs:
        xb = _be(x0) if group == 1 else _be(x1) + _be(x0)
        if compressed:
            for sign in (0, 0x20):
                add("curve", "x = %r, sign bit %#x" % ((x0, x1), sign), bytes([xb[0] | 0x80 | sign]) + xb[1:])
            continue
        if group == 1:
            y = P.fp_sqrt(x0 ** 3 + 4)
            ys = [_be(1), _be(P.P - 1)] if y is None else [_be(y), _be(P.P - y)]
        else:
            x = P.Fp2(x0, x1)
            y = P.fp2_sqrt(x * x * x + P.B2)
            ys = [_be(0) + _be(1), _be(0) + _be(P.P - 1)] if y is None else [_be(y.b) + _be(y.a), _be((-y).b) + _be((-y).a)]
        for i, yb in enumerate(ys):
            add("curve", "x = %r, y #%d" % ((x0, x1), i), xb + yb)
    assert all(len(c.data) == size for c in out)
    return out


def oracle_verdict(group, compressed, data):
    fn = {(1, True): P.g1_decompress, (2, True): P.g2_decompress, (1, False): P.g1_decode, (2, False): P.g2_decode}[(group, compressed)]
    return fn(data)


_VERDICTS = {}


def matrix(group, compressed):
    """[(Case, verdict, uncompressed bytes of the point or None)] with the oracle's verdict, computed once per process."""
    key = (group, compressed)
    if key not in _VERDICTS:
        rows = []
        for c in cases(group, compressed):
            v, pt = oracle_verdict(group, compressed, c.data)
            rows.append((c, v, _to_bytes(group, pt) if v == P.OK else None))
        _VERDICTS[key] = rows
    return _VERDICTS[key]


# ---------------------------------------------------------------- malformed point strings inside JSON records (tests/test_wire.py, tests/test_decoders.py)
WRONG_LENGTHS = (0, 1, 47, 49, 95, 97)


def bad_point_strings(group):
    """(kind, label, bytes): kind "length" -- strings of the lengths no compressed point of either group has (cut from / padded onto a valid point, so
    that a reader that ignored the length would find a point in them) -- and kind "point": the malformed infinities of the compressed form."""
    good = _compress(group, P.pt_mul_jac(P.G1 if group == 1 else P.G2, 7))
    out = [("length", "%d bytes" % n, (good + good + good)[:n]) for n in WRONG_LENGTHS]
    return out + [("point", label, data) for label, data in malformed_infinities(group, True)]


def point_paths(doc):
    """{1: [path, ...], 2: [...]}: where the compressed G1 (48-byte) and G2 (96-byte) strings of a parsed record sit, in document order."""
    found = {1: [], 2: []}

    def walk(v, path):
        if isinstance(v, dict):
            for k, x in v.items():
                walk(x, path + (k,))
        elif isinstance(v, list):
            for i, x in enumerate(v):
                walk(x, path + (i,))
        elif isinstance(v, bytes) and len(v) in (48, 96) and v[0] & 0x80:
            found[len(v) // 48].append(path)
    walk(doc, ())
    return found


def first_middle_last(paths):
    return list(dict.fromkeys([paths[0], paths[len(paths) // 2], paths[-1]]))


def replaced(doc, path, value):
    """A copy of the parsed record with the value at `path` replaced."""
    if not path:
        return value
    if isinstance(doc, dict):
        return {k: (replaced(x, path[1:], value) if k == path[0] else x) for k, x in doc.items()}
    return [replaced(x, path[1:], value) if i == path[0] else x for i, x in enumerate(doc)]


def message_class(exc):
    """The two kinds of refusal a reader has for a point string: its length, or what the decoder says about its 48 / 96 bytes."""
    text = str(exc)
    if "point is 48 bytes" in text or "point is 96 bytes" in text:
        return "length"
    if text.startswith("wire: bad point"):
        return "point"
    return "other: " + text


def check_reader_refuses_bad_point_strings(wire, reader, record):
    """Every point string of the record's first, middle and last G1 and G2 field, replaced by each bad string in turn: the reader (of `wire`, the
    module under test) raises ValueError of the right class.  -> the number of replacements tried."""
    doc = wire.loads(record)
    assert wire.dumps(doc) == record
    reader(record)                                                      # the record itself is read
    paths = point_paths(doc)
    tried = 0
    for group in (1, 2):
        assert paths[group], "the record holds no G%d point" % group
        for path in first_middle_last(paths[group]):
            for kind, label, bad in bad_point_strings(group):
                try:
                    reader(wire.dumps(replaced(doc, path, bad)))
                except ValueError as e:
                    assert message_class(e) == kind, (reader.__name__, path, label, str(e))
                else:
                    raise AssertionError("%s read a record whose %r is %s" % (reader.__name__, path, label))
                tried += 1
    return tried
