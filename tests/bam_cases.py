"""BAM test material (CPU): a writer for small BAM files whose BGZF seams fall where a test puts them (bgzf_cases.write), and the oracle of
`(no)boringbits --bam` — the rules of include/cornetto_accel.h (a restatement of `samtools depth -aa` and `samtools depth -Q 20 -aa`) in their
plainest form, one position at a time.  tests/test_bam_host.py pins the oracle with vectors worked out by hand."""
import random
import struct
import zlib

import numpy as np

import bgzf_cases

OPS = "MIDNSHP=X"
E_SHORT, E_TRUNC, E_FIELDS, E_REFID, E_CG, E_BGZF = 1, 2, 3, 4, 5, 6
SKIP_FLAGS = 0x704


# ---- writer ---------------------------------------------------------------------------------------------------------------------------------
def ops(text):
    """'2S5M2D' -> [(2, 'S'), (5, 'M'), (2, 'D')]"""
    out, num = [], ""
    for ch in text:
        if ch.isdigit():
            num += ch
        else:
            out.append((int(num), ch))
            num = ""
    assert num == ""
    return out


def pack_ops(cig):
    cig = ops(cig) if isinstance(cig, str) else cig
    return b"".join(struct.pack("<I", (n << 4) | (OPS.index(k) if isinstance(k, str) else k)) for n, k in cig)


def aux_cg(cig, count=None):
    """the CG:B,I field of a long-CIGAR record (count: the element count written, when it is to differ from the array's)"""
    body = pack_ops(cig)
    return b"CGBI" + struct.pack("<I", len(body) // 4 if count is None else count) + body


def record(ref_id, pos, cig=(), mapq=60, flag=0, l_seq=0, name=b"r", aux=b"", n_cigar=None, block_size=None, l_seq_field=None):
    """one alignment record, block_size included.  l_seq bases are written (as zeros); n_cigar / block_size / l_seq_field: the field as
    written, when it is to differ from the truth"""
    body = pack_ops(cig)
    n_ops = len(body) // 4
    assert n_ops <= 0xFFFF
    name = name + b"\0"
    data = struct.pack("<iiBBHHHIiii", ref_id, pos, len(name), mapq, 4680, n_ops if n_cigar is None else n_cigar, flag, l_seq if l_seq_field is None else l_seq_field, -1, -1,
                       0) + name + body + bytes((l_seq + 1) // 2) + bytes(l_seq) + aux
    return struct.pack("<i", len(data) if block_size is None else block_size) + data


def long_record(ref_id, pos, cig, l_seq=5, tag=True, **kw):
    """what htslib writes for more than 65535 operations: the placeholder `<l_seq>S<span>N`, the CIGAR in CG:B,I (tag=False: no such field)"""
    cig = ops(cig) if isinstance(cig, str) else cig
    span = sum(n for n, k in cig if k in "MDN=X")
    return record(ref_id, pos, [(l_seq, "S"), (span, "N")], l_seq=l_seq, aux=b"XAAx" + (aux_cg(cig) if tag else b"") + b"XZZabc\0", **kw)


def header(contigs, text=b"@HD\tVN:1.6\n"):
    out = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(contigs))
    for name, ln in contigs:
        nm = (name if isinstance(name, bytes) else name.encode()) + b"\0"
        out += struct.pack("<i", len(nm)) + nm + struct.pack("<i", ln)
    return out


def raw(contigs, records, **kw):
    """the inflated bytes of a BAM"""
    return header(contigs, **kw) + b"".join(records)


def bam(contigs, records, sizes=None, eof=True, **kw):
    """a BAM file; sizes: the inflated bytes of its BGZF blocks (bgzf_cases.write)"""
    return bgzf_cases.write(raw(contigs, records, **kw), sizes, eof=eof)


# ---- oracle ---------------------------------------------------------------------------------------------------------------------------------
class Result:
    """status 0: names, lens, total / mq (a uint16 array per contig), n_records, n_counted, n_clamped, recs; status -6: err = (kind, record, a, b)"""

    def __init__(self):
        self.status, self.err, self.names, self.lens, self.total, self.mq = 0, None, [], [], [], []
        self.n_records = self.n_counted = self.n_clamped = 0
        self.recs, self.header_bytes = [], 0


def _cap31(v):
    return min(v, 0x7FFFFFFF)


def parse_header(data):
    """-> (names, lens, header bytes); None when the bytes end inside the header; ValueError when they are no BAM header"""
    if data[:4] != b"BAM\1"[:len(data[:4])]:
        raise ValueError("magic")
    if len(data) < 8:
        return None
    l_text = struct.unpack_from("<i", data, 4)[0]
    if l_text < 0:
        raise ValueError("l_text")
    p = 8 + l_text
    if len(data) - p < 4:
        return None
    n_ref = struct.unpack_from("<i", data, p)[0]
    if n_ref < 0:
        raise ValueError("n_ref")
    p += 4
    names, lens = [], []
    for _ in range(n_ref):
        if len(data) - p < 4:
            return None
        l_name = struct.unpack_from("<i", data, p)[0]
        if l_name < 1:
            raise ValueError("l_name")
        p += 4
        if len(data) - p < l_name + 4:
            return None
        names.append(data[p:p + l_name].split(b"\0")[0].decode())
        p += l_name
        ln = struct.unpack_from("<i", data, p)[0]
        if ln < 0:
            raise ValueError("l_ref")
        lens.append(ln)
        p += 4
    return names, lens, p


def _find_cg(d, p):
    """the CG:B,I array among the auxiliary fields d[p:] -> list of op words, None (no such field), or (elements, room) when it runs past the record"""
    bs = len(d)
    while bs - p >= 3:
        tag, ty = d[p:p + 2], chr(d[p + 2])
        p += 3
        if ty in "AcC":
            sz = 1
        elif ty in "sS":
            sz = 2
        elif ty in "iIf":
            sz = 4
        elif ty in "ZH":
            while p < bs and d[p] != 0:
                p += 1
            if p >= bs:
                return None
            sz = 1
        elif ty == "B":
            if bs - p < 5:
                return None
            sub, cnt = chr(d[p]), struct.unpack_from("<I", d, p + 1)[0]
            p += 5
            if sub in "cC":
                es = 1
            elif sub in "sS":
                es = 2
            elif sub in "iIf":
                es = 4
            else:
                return None
            if tag == b"CG" and sub == "I":
                if cnt * 4 > bs - p:
                    return (_cap31(cnt), bs - p)
                return list(struct.unpack_from("<%dI" % cnt, d, p))
            sz = cnt * es
        else:
            return None
        if sz > bs - p:
            return None
        p += sz
    return None


def covered(pos, words):
    """the reference intervals [s, e) the M = X operations of a CIGAR (op words) cover from pos, and the span"""
    out, at = [], pos
    for w in words:
        n, k = w >> 4, w & 15
        if k in (0, 7, 8):
            if n:
                out.append((at, at + n))
            at += n
        elif k in (2, 3):
            at += n
    return out, at - pos


def oracle(data, min_mapq=20, skip_flags=SKIP_FLAGS, depth=True):
    """data: the inflated bytes of a BAM.  depth=False: no arrays (a header of billions of positions)"""
    r = Result()
    try:
        h = parse_header(data)
    except ValueError:
        r.status, r.err = -6, (7, -1, 0, 0)
        return r
    if h is None:
        r.status, r.err = -6, (E_TRUNC, -1, 0, -1)
        return r
    r.names, r.lens, p = h
    r.header_bytes = p
    n_ref = len(r.lens)
    acc = [[np.zeros(n, dtype=np.int64) for n in r.lens] for _ in range(2)] if depth else None
    i = 0

    def fail(kind, a, b):
        r.status, r.err = -6, (kind, i, a, b)
        return r
    while p < len(data):
        left = len(data) - p
        if left < 4:
            return fail(E_TRUNC, left, -1)
        bs = struct.unpack_from("<i", data, p)[0]
        if bs < 32:
            return fail(E_SHORT, bs, 0)
        if bs > left - 4:
            return fail(E_TRUNC, left, bs)
        d = data[p + 4:p + 4 + bs]
        ref_id, pos, l_read_name, mapq, _bin, n_cigar, flag, l_seq = struct.unpack_from("<iiBBHHHI", d, 0)
        fixed = 32 + l_read_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq
        if fixed > bs:
            return fail(E_FIELDS, _cap31(fixed), bs)
        if ref_id < -1 or ref_id >= n_ref:
            return fail(E_REFID, ref_id, n_ref)
        rec = dict(offset=p, ref_id=ref_id, pos=pos, mapq=mapq, flag=flag, counted=0, n_ops=0, span=0, bases=0)
        if ref_id >= 0 and (flag & skip_flags) == 0:
            words = list(struct.unpack_from("<%dI" % n_cigar, d, 32 + l_read_name))
            if n_cigar == 2 and words[0] & 15 == 4 and words[0] >> 4 == l_seq and words[1] & 15 == 3:
                cg = _find_cg(d, fixed)
                if isinstance(cg, tuple):
                    return fail(E_CG, cg[0], cg[1])
                if cg is not None:
                    words = cg
            ivls, span = covered(pos, words)
            n = r.lens[ref_id]
            bases = 0
            for s, e in ivls:
                s, e = min(max(s, 0), n), min(max(e, 0), n)
                bases += e - s
                if depth and e > s:
                    acc[0][ref_id][s:e] += 1
                    if mapq >= min_mapq:
                        acc[1][ref_id][s:e] += 1
            rec.update(counted=1, n_ops=len(words), span=span, bases=bases)
            r.n_counted += 1
        r.recs.append(rec)
        i += 1
        p += 4 + bs
    r.n_records = i
    if depth:
        for a in acc[0] + acc[1]:
            r.n_clamped += int((a > 65535).sum())
        r.total = [np.minimum(a, 65535).astype(np.uint16) for a in acc[0]]
        r.mq = [np.minimum(a, 65535).astype(np.uint16) for a in acc[1]]
    return r


def bedgraphs(r):
    """the per-base bedgraph pair of an oracle result: what `samtools depth -aa | awk` gives for the same coverage"""
    out = []
    for arrs in (r.total, r.mq):
        lines = []
        for name, a in zip(r.names, arrs):
            lines.extend("%s\t%d\t%d\t%d\n" % (name, i, i + 1, v) for i, v in enumerate(a.tolist()))
        out.append("".join(lines).encode())
    return out


def checksum(arrs):
    """CRC-32 over the arrays of all contigs (tools/sim/bam_sim.cc prints the same)"""
    c = 0
    for a in arrs:
        c = zlib.crc32(np.ascontiguousarray(a, dtype="<u2").tobytes(), c)
    return c & 0xFFFFFFFF


# ---- cases ----------------------------------------------------------------------------------------------------------------------------------
ALL_OPS = "3M2I4D1=2X5N3P2M"          # every kind that may stand inside a CIGAR


def cigar_cases():
    """name -> (contigs, records)"""
    c1 = [("ctgA", 400), ("ctgB", 90)]
    many = lambda n: [(1 + (i % 3), "MID"[i % 3] if i % 7 else "M") for i in range(n)]
    cases = {
        "handworked": (c1, [record(0, 3, "2S5M2D3M1I4M3H")]),
        "all_ops": (c1, [record(0, 10, "4H2S" + ALL_OPS + "3S2H"), record(1, 0, ALL_OPS)]),
        "zero_len": (c1, [record(0, 5, "0M3M0D0I2M0N4M0S"), record(0, 7, "0M"), record(1, 2, "0D0N")]),
        "no_cigar": (c1, [record(0, 5), record(0, 6, "3M")]),
        "leading_del": (c1, [record(0, 5, "2D3M2N"), record(0, 5, "3D"), record(0, 9, "1M2D3N1M")]),
        "ops_9_15": (c1, [record(0, 5, [(3, "M"), (4, 9), (2, 15), (2, "M")])]),
    }
    for n in (63, 64, 65, 128, 200):
        cases["ops_%d" % n] = (c1, [record(0, 1, many(n)), record(1, 3, [(1, "M"), (1, "D")] * (n // 2) + [(1, "M")] * (n % 2))])
    big = [(1, "M"), (1, "I")] * 34000 + [(2, "D"), (3, "M")] * 1000
    cases["cg_tag"] = ([("ctgA", 40000), ("ctgB", 90)], [record(0, 2, "5M"), long_record(0, 100, big), record(1, 0, "5M")])
    assert len(big) == 70000
    cases["cg_missing"] = (c1, [long_record(0, 10, "20M5D20M", tag=False), record(0, 0, "5M")])
    cases["cg_small"] = (c1, [long_record(0, 10, "20M5D20M"), long_record(0, 10, "7M", l_seq=4, l_seq_field=4)])
    cases["cg_not_placeholder"] = (c1, [record(0, 10, "5S30N", l_seq=4, aux=aux_cg("7M"))])       # l_seq differs from the S: the two ops as they stand
    return cases


def position_cases():
    c = [("a", 100), ("b", 50)]
    recs = [record(0, 95, "10M"), record(0, 99, "1M"), record(0, 99, "5M"), record(0, 100, "5M"), record(0, 200, "5M"), record(0, -1, "3M"), record(0, -5, "3M"),
            record(1, 45, "2M10D2M"), record(1, 40, "5M3D10M"), record(-1, -1), record(-1, 5, "5M"), record(1, 0x7FFFFFF0, "100M")]
    flags = [record(0, 10, "5M", flag=f) for f in (0x4, 0x100, 0x200, 0x400, 0x1, 0x10, 0x800, 0x704, 0)]
    mapqs = [record(1, 10, "5M", mapq=q) for q in (0, 19, 20, 21, 255)]
    return {"clip": (c, recs), "flags": (c, flags), "mapq": (c, mapqs)}


def contig_cases(tile):
    cases = {
        "empty_contigs": ([("e0", 0), ("a", 10), ("e1", 0), ("e2", 0), ("one", 1), ("b", 64), ("e3", 0)],
                          [record(0, 0, "5M"), record(1, 0, "10M"), record(1, 9, "1M"), record(2, 0, "1M"), record(4, 0, "1M"), record(4, 0, "3M"), record(5, 0, "64M"),
                           record(5, 63, "5M"), record(6, 0, "4M")]),
        "no_contigs": ([], [record(-1, -1), record(-1, 0, "5M")]),
        "no_records": ([("a", 70), ("b", 3)], []),
    }
    rng = random.Random(7)
    contigs, recs = [], []
    for i in range(300):
        ln = max(1, tile * rng.choice((0, 1, 1, 2)) + rng.choice((-1, 0, 1)) + (0 if i % 5 else 64 * rng.randrange(3)))
        contigs.append(("t%d" % i, ln))
        for _ in range(2):
            e = min(ln, max(1, tile * rng.choice((1, 2)) + rng.choice((-1, 0, 1))))
            s = rng.randrange(0, e)
            recs.append(record(i, s, "%dM" % (e - s), mapq=rng.choice((5, 60))))
        recs.append(record(i, max(0, ln - 3), "6M"))
    cases["tiles"] = (contigs, recs)
    return cases


def random_case(seed, n_ctg=None, n_reads=None):
    rng = random.Random(seed)
    n_ctg = n_ctg if n_ctg is not None else rng.randrange(1, 6)
    contigs = [("c%d" % i, rng.choice((1, 17, 64, 500, 3000, 9000))) for i in range(n_ctg)]
    indel = rng.choice((0.0, 0.04, 0.3))
    recs = []
    for _ in range(n_reads if n_reads is not None else rng.randrange(1, 60)):
        c = rng.randrange(n_ctg)
        want = rng.choice((1, 30, 400, 2500))
        cig = [(rng.randrange(1, 40), "S")] if rng.random() < 0.3 else []
        while want > 0:
            n = min(want, rng.randrange(1, 60))
            cig.append((n, rng.choice("M=X")))
            want -= n
            if rng.random() < indel * 10:
                cig.append((rng.randrange(0, 12), rng.choice("IDDNP")))
        recs.append(record(c, rng.randrange(-3, contigs[c][1] + 3), cig, mapq=rng.choice((0, 19, 20, 60)), flag=rng.choice((0, 0, 0, 16, 0x100, 0x400, 0x800)),
                           l_seq=rng.choice((0, 0, 3)), aux=rng.choice((b"", b"NMC\5", b"XSZhello\0RGZx\0"))))
    return contigs, recs


def valid_cases(tile):
    """every valid case of this file: name -> (contigs, records)"""
    cases = {}
    cases.update(cigar_cases())
    cases.update(position_cases())
    cases.update(contig_cases(tile))
    for seed in range(12):
        cases["random_%d" % seed] = random_case(seed)
    return cases


def record_sizes(data):
    """[(offset, bytes)] of the records of the valid inflated BAM `data`"""
    p, out = parse_header(data)[2], []
    while p < len(data):
        n = 4 + struct.unpack_from("<i", data, p)[0]
        out.append((p, n))
        p += n
    return out


def bad_cases():
    """name -> (inflated bytes, (kind, record, a, b))"""
    c = [("a", 100), ("b", 50)]
    good = [record(0, 1, "5M"), record(1, 2, "5M")]
    whole = raw(c, good + [record(0, 3, "4M")])
    cg_rec = record(0, 10, "5S30N", l_seq=5, aux=aux_cg("7M3D2M", count=9))
    cases = {
        "short_block": (raw(c, good + [record(0, 3, "4M", block_size=31), record(0, 0, "1M")]), (E_SHORT, 2, 31, 0)),
        "negative_block": (raw(c, good + [record(0, 3, "4M", block_size=-5)]), (E_SHORT, 2, -5, 0)),
        "cut_record": (whole[:-7], (E_TRUNC, 2, len(record(0, 3, "4M")) - 7, len(record(0, 3, "4M")) - 4)),
        "cut_block_size": (whole + b"\x40\0", (E_TRUNC, 3, 2, -1)),
        "fields_cigar": (raw(c, good + [record(0, 3, "4M", n_cigar=200)]), (E_FIELDS, 2, 32 + 2 + 800, 32 + 2 + 4)),
        "fields_l_seq": (raw(c, good + [record(0, 3, "4M", l_seq_field=0xFFFFFFFF)]), (E_FIELDS, 2, 0x7FFFFFFF, 32 + 2 + 4)),
        "refid_high": (raw(c, [record(2, 3, "4M")] + good), (E_REFID, 0, 2, 2)),
        "refid_low": (raw(c, good + [record(-2, 3, "4M")]), (E_REFID, 2, -2, 2)),
        "refid_unmapped_flag": (raw(c, good + [record(7, 3, "4M", flag=4)]), (E_REFID, 2, 7, 2)),
        "cg_past_record": (raw(c, good + [cg_rec]), (E_CG, 2, 9, 12)),
        "first_error_wins": (raw(c, [record(0, 1, "5M"), record(5, 1, "5M"), record(0, 3, "4M", block_size=8)]), (E_REFID, 1, 5, 2)),
    }
    return cases
