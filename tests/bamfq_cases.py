"""`seq --bam` test material (CPU): a writer for BAM records with bases, qualities and auxiliary fields (the header and the BGZF container
are those of bam_cases / bgzf_cases), and the oracle of `cornetto seq --bam` — the rules of include/cornetto_accel.h in their plainest form,
one record and one byte at a time.  tests/test_bamfq_host.py pins the oracle with vectors worked out by hand."""
import random
import struct
import zlib

import bam_cases
import bgzf_cases

CODES = "=ACMGRSVTWYHKDBN"
COMP = "=TGKCYSBAWRDMHVN"
E_SHORT, E_TRUNC, E_FIELDS, E_REFID, E_BGZF = 1, 2, 3, 4, 6
HEADER = bam_cases.header([])          # a basecaller's BAM has no reference contig


# ---- writer ---------------------------------------------------------------------------------------------------------------------------------
def pack_bases(bases):
    """bases: a string over CODES, or a list of nibble codes"""
    nib = [CODES.index(c) for c in bases] if isinstance(bases, str) else list(bases)
    nib2 = nib + [0] * (len(nib) & 1)
    return bytes((nib2[i] << 4) | nib2[i + 1] for i in range(0, len(nib2), 2))


def record(name=b"r", bases="", quals=None, flag=4, aux=b"", ref_id=-1, no_name=False, block_size=None, l_seq_field=None, n_cigar=0):
    """one record, block_size included.  quals: bytes of len(bases) (None: absent, 0xFF each); no_name: l_read_name 0 and no name bytes;
    block_size / l_seq_field / n_cigar: the field as written, when it is to differ from the truth"""
    l_seq = len(bases)
    quals = bytes([0xFF]) * l_seq if quals is None else bytes(quals)
    assert len(quals) == l_seq
    nm = b"" if no_name else name + b"\0"
    assert len(nm) <= 255
    data = struct.pack("<iiBBHHHIiii", ref_id, -1, len(nm), 0, 4680, n_cigar, flag, l_seq if l_seq_field is None else l_seq_field, -1, -1, 0)
    data += nm + pack_bases(bases) + quals + aux
    return struct.pack("<i", len(data) if block_size is None else block_size) + data


def aux_int(tag, ty, value):
    return tag + ty.encode() + struct.pack("<" + {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I"}[ty], value)


def raw(records, header=HEADER):
    return header + b"".join(records)


def bam(records, sizes=None, eof=True, header=HEADER):
    return bgzf_cases.write(raw(records, header), sizes, eof=eof)


# ---- oracle ---------------------------------------------------------------------------------------------------------------------------------
class Result:
    """status 0 or -6 (err = (kind, record, a, b)); text: the FASTQ text (of the records in front of the failing one); stats: reads and bases
    of `total reads`, reads and bases of `reads >= min_len`; recs: one dict per record taken"""

    def __init__(self):
        self.status, self.err, self.text, self.stats, self.recs = 0, None, b"", [0, 0, 0, 0], []


def find_dx(d, p):
    """the first integer field dx among the auxiliary fields d[p:] -> its value, or None"""
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
                sz = cnt
            elif sub in "sS":
                sz = 2 * cnt
            elif sub in "iIf":
                sz = 4 * cnt
            else:
                return None
        else:
            return None
        if sz > bs - p:
            return None
        if tag == b"dx" and ty in "cCsSiI":
            return struct.unpack_from("<" + {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I"}[ty], d, p)[0]
        p += sz
    return None


def fastq_of(d):
    """the text of one record's data (behind block_size), its checks passed"""
    l_read_name, n_cigar, flag, l_seq = d[8], struct.unpack_from("<H", d, 12)[0], struct.unpack_from("<H", d, 14)[0], struct.unpack_from("<I", d, 16)[0]
    name = d[32:32 + max(l_read_name - 1, 0)]
    p = 32 + l_read_name + 4 * n_cigar
    seq, qual = d[p:p + (l_seq + 1) // 2], d[p + (l_seq + 1) // 2:p + (l_seq + 1) // 2 + l_seq]
    nib = []
    for i in range(l_seq):
        b = seq[i >> 1]
        nib.append(b & 15 if i & 1 else b >> 4)
    if l_seq and qual[0] == 0xFF:
        q = [ord('"')] * l_seq
    else:
        q = [min(x, 93) + 33 for x in qual]
    if flag & 0x10:
        bases = "".join(COMP[x] for x in reversed(nib))
        q.reverse()
    else:
        bases = "".join(CODES[x] for x in nib)
    return b"@" + name + b"\n" + bases.encode() + b"\n+\n" + bytes(q) + b"\n"


def oracle(data, min_len=0, duplex=False):
    """data: the inflated bytes of a BAM"""
    r = Result()
    try:
        h = bam_cases.parse_header(data)
    except ValueError:
        r.status, r.err = -6, (7, -1, 0, 0)
        return r
    if h is None:
        r.status, r.err = -6, (E_TRUNC, -1, 0, -1)
        return r
    n_ref, p = len(h[1]), h[2]
    out, i = [], 0

    def fail(kind, a, b):
        r.status, r.err, r.text = -6, (kind, i, a, b), b"".join(out)
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
        ref_id, _pos, l_read_name, _mapq, _bin, n_cigar, flag, l_seq = struct.unpack_from("<iiBBHHHI", d, 0)
        fixed = 32 + l_read_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq
        if fixed > bs:
            return fail(E_FIELDS, min(fixed, 0x7FFFFFFF), bs)
        if ref_id < -1 or ref_id >= n_ref:
            return fail(E_REFID, ref_id, n_ref)
        rec = dict(offset=p, l_seq=l_seq, flag=flag, name_len=max(l_read_name - 1, 0), kept=0)
        if flag & 0x900:
            rec["kept"] = -1
        else:
            r.stats[0] += 1
            r.stats[1] += l_seq
            if l_seq >= min_len and (not duplex or find_dx(d, fixed) == 1):
                rec["kept"] = 1
                r.stats[2] += 1
                r.stats[3] += l_seq
                out.append(fastq_of(d))
        r.recs.append(rec)
        i += 1
        p += 4 + bs
    r.text = b"".join(out)
    return r


def summary(r, min_len):
    """the two stderr lines of `seq`"""
    return ("total reads: %d\t%d bases\t%.2f Gbases\nreads >= %d: %d\t%d bases\t%.2f Gbases\n" %
            (r.stats[0], r.stats[1], r.stats[1] / 1e9, min_len, r.stats[2], r.stats[3], r.stats[3] / 1e9)).encode()


def line(r):
    """what tools/sim/bamfq_sim.cc prints for a case"""
    if r.status:
        return "%d %d %d %d %d %d %d" % ((r.status,) + tuple(r.err) + (len(r.text), zlib.crc32(r.text) & 0xFFFFFFFF))
    return "0 0 0 0 0 %d %d %d %d %d %d" % (len(r.text), zlib.crc32(r.text) & 0xFFFFFFFF, r.stats[0], r.stats[1], r.stats[2], r.stats[3])


def record_sizes(data):
    """[(offset, bytes)] of the records of the valid inflated BAM `data`"""
    return bam_cases.record_sizes(data)


# ---- cases ----------------------------------------------------------------------------------------------------------------------------------
def _read(rng, n, **kw):
    return record(bases="".join(rng.choice("ACGT") for _ in range(n)), quals=bytes(rng.randrange(0, 60) for _ in range(n)), **kw)


LENGTHS = (0, 1, 2, 15, 16, 17, 31, 32, 33, 257)
DX_TYPES = "cCsSiI"


def valid_cases():
    """name -> (records, [(min_len, duplex), ...]): the runs a case is taken through"""
    rng = random.Random(3)
    plain, both = [(0, False)], [(0, False), (0, True)]
    cases = {}
    recs = []
    for n in LENGTHS:
        for flag in (4, 0x14):
            recs.append(_read(rng, n, name=b"len%d_%x" % (n, flag), flag=flag))
    cases["l_seq"] = (recs, [(0, False), (16, False), (17, False), (258, False)])
    cases["names"] = ([_read(rng, 20, name=b"n" * k, flag=f) for k in (0, 1, 14, 15, 16, 254) for f in (4, 0x14)] +
                      [_read(rng, 20, no_name=True), _read(rng, 0, no_name=True), _read(rng, 33, no_name=True, flag=0x14)], plain)
    cases["alignment"] = ([_read(rng, 40 + (k % 3), name=b"x" * k, flag=0x10 * (k & 1) | 4) for k in range(34)], plain)
    codes = list(range(16)) + list(range(15, -1, -1)) + [3, 7, 11]
    cases["nibbles"] = ([record(b"fwd", codes, bytes(range(35))), record(b"rev", codes, bytes(range(35)), flag=0x14), record(b"odd", codes[:17], bytes(17), flag=0x14)], plain)
    q = [0, 93, 94, 254, 255, 1, 92, 95, 127, 128, 200, 33, 0, 93, 94, 254, 255, 40, 41, 42]
    cases["quals"] = ([record(b"q", "ACGT" * 5, bytes(q)), record(b"qr", "ACGT" * 5, bytes(q), flag=0x14), record(b"absent", "ACGTN" * 7), record(b"absent_r", "ACGTN" * 7, flag=0x14),
                       record(b"ff_first", "A" * 18, bytes([0xFF] + [7] * 17)), record(b"ff_later", "C" * 18, bytes([7, 0xFF] + [9] * 16)), record(b"one_absent", "G")], plain)
    recs = []
    for ty in DX_TYPES:
        for v in (1, 0, -1):
            if v < 0 and ty in "CSI":
                v = {"C": 255, "S": 65535, "I": 0xFFFFFFFF}[ty]
            recs.append(_read(rng, 24, name=b"dx_%s_%d" % (ty.encode(), v & 0xFF), aux=aux_int(b"dx", ty, v)))
    recs += [_read(rng, 24, name=b"dx_Z", aux=b"dxZ1\0"), _read(rng, 24, name=b"dx_f", aux=b"dxf" + struct.pack("<f", 1.0)), _read(rng, 24, name=b"dx_A", aux=b"dxA1"),
             _read(rng, 24, name=b"dx_Z_then_int", aux=b"dxZ1\0" + aux_int(b"dx", "c", 1)), _read(rng, 24, name=b"dx_300", aux=aux_int(b"dx", "s", 257))]
    cases["dx_values"] = (recs, both)
    one = aux_int(b"dx", "c", 1)
    arr = b"mvBc" + struct.pack("<I", 5) + bytes(5)
    cases["dx_positions"] = ([
        _read(rng, 20, name=b"behind_B", aux=arr + one), _read(rng, 20, name=b"behind_Z", aux=b"RGZgroup\0" + one), _read(rng, 20, name=b"behind_H", aux=b"xhH1AE3\0" + one),
        _read(rng, 20, name=b"behind_all", aux=b"qsi" + struct.pack("<i", 20) + b"duf" + struct.pack("<f", 2.5) + arr + b"stA+" + b"BsBS" + struct.pack("<I", 2) + bytes(4) + one),
        _read(rng, 20, name=b"absent", aux=arr), _read(rng, 20, name=b"no_aux"),
        _read(rng, 20, name=b"behind_bad_type", aux=b"zz?1" + one), _read(rng, 20, name=b"behind_bad_sub", aux=b"zzBx" + struct.pack("<I", 1) + b"\0" + one),
        _read(rng, 20, name=b"behind_open_Z", aux=b"RGZgroup" + one[:2]), _read(rng, 20, name=b"behind_long_B", aux=b"mvBi" + struct.pack("<I", 1 << 30) + one),
        _read(rng, 20, name=b"cut_value", aux=aux_int(b"dx", "i", 1)[:5]), _read(rng, 20, name=b"cut_type", aux=b"dx"), _read(rng, 20, name=b"cut_s", aux=b"dxs\1"),
        _read(rng, 20, name=b"whole", aux=one)], both)
    cases["flags"] = ([_read(rng, 30, name=b"f%x" % f, flag=f, aux=one) for f in (0x100, 0x800, 0x4, 0x10, 0x900, 0x110, 0x0, 0x814, 0x1, 0x400)], both + [(31, False)])
    cases["nothing_kept"] = ([_read(rng, 10 + k, name=b"s%d" % k) for k in range(30)], [(1000, False), (0, True)])
    cases["everything_kept"] = ([_read(rng, 10 + k, name=b"s%d" % k, aux=one) for k in range(30)], both)
    # records of about 100 bytes; the middle third is too short: at a window of a few hundred bytes whole windows print nothing
    cases["window_dropped"] = ([_read(rng, 50 if not 20 <= k < 40 else 10, name=b"w%d" % k) for k in range(60)], [(30, False)])
    cases["many_small"] = ([_read(rng, rng.randrange(0, 41), name=b"%d" % k, flag=rng.choice((4, 0x14, 0x104))) for k in range(10000)], [(0, False), (20, False)])
    cases["one_long"] = ([_read(rng, 20, name=b"a"), _read(rng, 200000, name=b"long_fwd"), _read(rng, 200001, name=b"long_rev", flag=0x14), record(b"long_absent", "ACGTAC" * 5000)],
                         [(0, False), (30000, False)])
    return cases


def seam_case():
    """a file and the block sizes that plant BGZF seams inside block_size, the fixed fields, the name, the bases, the qualities and the dx field"""
    rng = random.Random(8)
    recs = [_read(rng, 61 + k, name=b"seam_%d" % k, flag=(4, 0x14)[k & 1], aux=b"RGZg\0" + aux_int(b"dx", "i", k % 2)) for k in range(12)]
    data = raw(recs)
    cuts = []
    for k, (off, n) in enumerate(record_sizes(data)):
        l_seq = 61 + k
        name_at, seq_at = off + 36, off + 36 + len(b"seam_%d" % k) + 1
        qual_at = seq_at + (l_seq + 1) // 2
        cuts.append([off + 2, off + 20, name_at + 3, seq_at + 9, qual_at + 30, off + n - 2][k % 6])
    sizes = [b - a for a, b in zip([0] + cuts, cuts)]
    return recs, sizes


def bad_cases():
    """name -> (inflated bytes, (kind, record, a, b))"""
    rng = random.Random(4)
    good = [_read(rng, 40, name=b"g0"), _read(rng, 41, name=b"g1", flag=0x14)]
    last = _read(rng, 20, name=b"last")
    whole = raw(good + [last])
    n_last = len(last)
    return {
        "short_block": (raw(good + [record(b"x", "ACGT", block_size=31), last]), (E_SHORT, 2, 31, 0)),
        "negative_block": (raw(good + [record(b"x", "ACGT", block_size=-5)]), (E_SHORT, 2, -5, 0)),
        "cut_record": (whole[:-7], (E_TRUNC, 2, n_last - 7, n_last - 4)),
        "cut_block_size": (whole + b"\x40\0", (E_TRUNC, 3, 2, -1)),
        "fields_l_seq": (raw(good + [record(b"x", "ACGT", bytes(4), l_seq_field=0xFFFFFFFF)]), (E_FIELDS, 2, 0x7FFFFFFF, 32 + 2 + 2 + 4)),
        "fields_l_seq_small": (raw(good + [record(b"x", "ACGT", bytes(4), l_seq_field=6), last]), (E_FIELDS, 2, 32 + 2 + 3 + 6, 32 + 2 + 2 + 4)),
        "fields_cigar": (raw(good + [record(b"x", "ACGT", bytes(4), n_cigar=9)]), (E_FIELDS, 2, 32 + 2 + 36 + 2 + 4, 32 + 2 + 2 + 4)),
        "refid_high": (raw([record(b"x", "ACGT", ref_id=0)] + good), (E_REFID, 0, 0, 0)),
        "refid_low": (raw(good + [record(b"x", "ACGT", ref_id=-2)]), (E_REFID, 2, -2, 0)),
        "refid_secondary": (raw(good + [record(b"x", "ACGT", ref_id=3, flag=0x100)]), (E_REFID, 2, 3, 0)),
        "first_error_wins": (raw([good[0], record(b"x", "ACGT", ref_id=5), record(b"y", "ACGT", block_size=8)]), (E_REFID, 1, 5, 0)),
    }
