// bamfq.hpp — one BAM record as FASTQ text, behind cornetto_bamfq_*() (include/cornetto_accel.h states the rules): ONE source for the device
// (bamfq.hip: a thread per record in the size pass, a thread per 16 output bytes in the text kernel) and for the CPU (tools/sim/bamfq_sim.cc:
// the same statements under the host sanitizers against the Python oracle; cli/host_backend.c's rules are the same, in C).  Nothing here
// needs a lane shim: no statement looks at another lane.
// Bounds come from the code, never from the input: cnq_size() reads inside [rec, rec + 4 + block_size) only — the fixed-field equation is
// checked before name, bases or qualities are touched, every auxiliary field against the record's end before it is read —, and cnq_chunk()
// reads the name, bases and qualities of records that have passed cnq_size(), the offset tables inside [0, n] and nothing else.
// Records are not aligned in the text: fields are put together from byte loads, the 8 bytes of a fast path are fetched with memcpy.
#pragma once
#include "bam.hpp"

// what cnq_size() found
struct CnqOut {
    int32_t l_seq, flag, name_len;
    int32_t kept;      // 1: printed; 0: too short or no dx:1; -1: passed over (SECONDARY / SUPPLEMENTARY): in neither count
    uint32_t size;     // bytes of its text: name_len + 2 l_seq + 6, or 0
};

// The integer field dx among the auxiliary fields data[p .. bs) -> 1 and *val, or 0: none (fields that do not parse end the search; a dx of
// another type is no tag and the search goes on behind it).  The walk of cnb_find_cg().
CNB_HD static inline int cnq_find_dx(const uint8_t *data, int64_t p, int64_t bs, int64_t *val)
{
    while (bs - p >= 3) {
        const uint8_t t0 = data[p], t1 = data[p + 1], ty = data[p + 2];
        p += 3;
        int64_t sz;
        if (ty == 'A' || ty == 'c' || ty == 'C') sz = 1;
        else if (ty == 's' || ty == 'S') sz = 2;
        else if (ty == 'i' || ty == 'I' || ty == 'f') sz = 4;
        else if (ty == 'Z' || ty == 'H') {
            while (p < bs && data[p] != 0) ++p;
            if (p >= bs) return 0;
            sz = 1;
        } else if (ty == 'B') {
            if (bs - p < 5) return 0;
            const uint8_t sub = data[p];
            const int64_t cnt = (int64_t)cnb_u32(data + p + 1);
            p += 5;
            int64_t es;
            if (sub == 'c' || sub == 'C') es = 1;
            else if (sub == 's' || sub == 'S') es = 2;
            else if (sub == 'i' || sub == 'I' || sub == 'f') es = 4;
            else return 0;
            sz = cnt * es;
        } else return 0;
        if (sz > bs - p) return 0;
        if (t0 == 'd' && t1 == 'x' && ty != 'A' && ty != 'f' && ty != 'Z' && ty != 'H' && ty != 'B') {
            if (ty == 'c') *val = (int8_t)data[p];
            else if (ty == 'C') *val = data[p];
            else if (ty == 's') *val = (int16_t)cnb_u16(data + p);
            else if (ty == 'S') *val = (int64_t)cnb_u16(data + p);
            else if (ty == 'i') *val = (int32_t)cnb_u32(data + p);
            else *val = (int64_t)cnb_u32(data + p);
            return 1;
        }
        p += sz;
    }
    return 0;
}

// rec: the record's block_size field, the record wholly readable (cnb_frame).  The checks (kinds 3 and 4), then the flag, length and dx rules.
CNB_HD static inline int cnq_size(const uint8_t *rec, int32_t n_ref, int64_t min_len, int duplex, CnqOut &o, CnbErr &e)
{
    const int64_t bs = (int64_t)(int32_t)cnb_u32(rec);
    const uint8_t *data = rec + 4;
    const int32_t ref_id = (int32_t)cnb_u32(data);
    const int64_t l_read_name = data[8], n_cigar = cnb_u16(data + 12), l_seq = (int64_t)cnb_u32(data + 16);
    o.flag = (int32_t)cnb_u16(data + 14);
    o.l_seq = cnb_cap31(l_seq);
    o.name_len = l_read_name ? (int32_t)l_read_name - 1 : 0;
    o.kept = 0;
    o.size = 0;
    e.kind = CNB_OK;
    e.a = e.b = 0;
    const int64_t fixed = 32 + l_read_name + 4 * n_cigar + (l_seq + 1) / 2 + l_seq;
    if (fixed > bs) {
        e.kind = CNB_FIELDS;
        e.a = cnb_cap31(fixed);
        e.b = (int32_t)bs;
        return e.kind;
    }
    if (ref_id < -1 || ref_id >= n_ref) {
        e.kind = CNB_REFID;
        e.a = ref_id;
        e.b = n_ref;
        return e.kind;
    }
    if (o.flag & 0x900) {
        o.kept = -1;
        return CNB_OK;
    }
    if (l_seq < min_len) return CNB_OK;
    if (duplex) {
        int64_t v = 0;
        if (!cnq_find_dx(data, fixed, bs, &v) || v != 1) return CNB_OK;
    }
    o.kept = 1;
    o.size = (uint32_t)(o.name_len + 2 * l_seq + 6);      // (below 2^32: 1.5 l_seq <= block_size < 2^31)
    return CNB_OK;
}

// ---- the text -----------------------------------------------------------------------------------------------------------------------------
// The text of a window is, for every record r of its table in order, size[r] bytes: '@' name '\n' bases '\n' '+' '\n' qualities '\n'.
// out[r] is the text offset of record r (an exclusive scan of the sizes), out[n] the length of the text.
struct CnqSrc {
    const uint8_t *text;    // the window
    const uint32_t *off;    // [n] the records' block_size fields
    const uint32_t *out;    // [n + 1]
    int64_t n;
};

// a record that is printed, as the text kernel needs it
struct CnqRec {
    const uint8_t *name, *seq, *qual;
    int64_t L, S;       // name bytes, bases
    int rev, no_qual;
};

CNB_HD static inline CnqRec cnq_rec(const uint8_t *rec)
{
    const uint8_t *data = rec + 4;
    const int64_t l_read_name = data[8], n_cigar = cnb_u16(data + 12);
    CnqRec r;
    r.S = (int64_t)cnb_u32(data + 16);
    r.L = l_read_name ? l_read_name - 1 : 0;
    r.rev = (cnb_u16(data + 14) & 0x10) != 0;
    r.name = data + 32;
    r.seq = r.name + l_read_name + 4 * n_cigar;
    r.qual = r.seq + (r.S + 1) / 2;
    r.no_qual = r.S > 0 && r.qual[0] == 0xFF;
    return r;
}

// "=ACMGRSVTWYHKDBN" and its complement "=TGKCYSBAWRDMHVN" as two 64-bit words each (byte k of word k >> 3)
#define CNQ_FWD_LO 0x565352474D43413Dull
#define CNQ_FWD_HI 0x4E42444B48595754ull
#define CNQ_REV_LO 0x425359434B47543Dull
#define CNQ_REV_HI 0x4E56484D44525741ull

CNB_HD static inline uint8_t cnq_base(uint32_t nib, int rev)
{
    const uint64_t w = nib < 8 ? (rev ? CNQ_REV_LO : CNQ_FWD_LO) : (rev ? CNQ_REV_HI : CNQ_FWD_HI);
    return (uint8_t)(w >> (8 * (nib & 7)));
}

CNB_HD static inline uint8_t cnq_byte(const CnqRec &r, int64_t k)      // byte k of the record's text, k < L + 2 S + 6
{
    if (k == 0) return '@';
    k -= 1;
    if (k < r.L) return r.name[k];
    k -= r.L;
    if (k == 0) return '\n';
    k -= 1;
    if (k < r.S) {
        const int64_t j = r.rev ? r.S - 1 - k : k;
        const uint8_t b = r.seq[j >> 1];
        return cnq_base((j & 1) ? (b & 15u) : (b >> 4), r.rev);
    }
    k -= r.S;
    if (k < 3) return k == 1 ? '+' : '\n';
    k -= 3;
    if (k < r.S) {
        if (r.no_qual) return '"';
        const uint8_t q = r.qual[r.rev ? r.S - 1 - k : k];
        return (uint8_t)((q > 93 ? 93 : q) + 33);
    }
    return '\n';
}

// largest r in [lo, hi] with out[r] <= p (records without text share their offset with the next one: the one found has text when p < out[n])
CNB_HD static inline int64_t cnq_find(const uint32_t *out, int64_t lo, int64_t hi, int64_t p)
{
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if ((int64_t)out[mid] <= p) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

CNB_HD static inline uint64_t cnq_load8(const uint8_t *p)
{
    uint64_t w;
    __builtin_memcpy(&w, p, 8);
    return w;
}

CNB_HD static inline uint64_t cnq_bswap8(uint64_t x) { return __builtin_bswap64(x); }

// min(q, 93) + 33 in every byte: bit 7 of ((q & 0x7F) + 34) | q is set iff q >= 94; no carry leaves a byte (0x7F + 0x22 = 0xA1, 93 + 33 = 126)
CNB_HD static inline uint64_t cnq_phred8(uint64_t x)
{
    const uint64_t t = (((x & 0x7F7F7F7F7F7F7F7Full) + 0x2222222222222222ull) | x) & 0x8080808080808080ull;
    const uint64_t m = (t >> 7) * 0xFFull;
    return ((x & ~m) | (0x5D5D5D5D5D5D5D5Dull & m)) + 0x2121212121212121ull;
}

// The bytes [p, p + m) of the text, m in 1 .. 16 and p + m <= out[n], as the low m bytes of v[0], v[1] (little endian); the rest is 0 or
// bytes of the fast path that the caller does not keep.  [r0, r1]: records that hold every byte of the range (a tile's, found once).
// A chunk of 16 bytes inside the bases or inside the qualities of one record is made from 9 or 16 source bytes, mirrored for a reverse-strand
// record; any other chunk byte by byte.
CNB_HD static inline void cnq_chunk(const CnqSrc &A, int64_t r0, int64_t r1, int64_t p, int m, uint64_t v[2])
{
    int64_t ri = cnq_find(A.out, r0, r1, p);
    CnqRec r = cnq_rec(A.text + A.off[ri]);
    int64_t o = A.out[ri];
    const int64_t k0 = p - o;
    if (m == 16) {
        const int64_t b0 = k0 - (2 + r.L);             // base index of the chunk's first byte
        if (b0 >= 0 && b0 + 16 <= r.S) {
            const int64_t j0 = r.rev ? r.S - 16 - b0 : b0;      // the lowest nibble of the 16
            const uint64_t w = cnq_load8(r.seq + (j0 >> 1));
            const uint32_t x = r.seq[(j0 >> 1) + 8];            // (inside the record: (j0 >> 1) + 8 <= S / 2, and S qualities follow the bases)
            const uint64_t lo = r.rev ? CNQ_REV_LO : CNQ_FWD_LO, hi = r.rev ? CNQ_REV_HI : CNQ_FWD_HI;
            const int odd = (int)(j0 & 1);
            v[0] = v[1] = 0;
            for (int i = 0; i < 16; ++i) {      // (a constant trip count: unrolled, every shift a constant but the table's)
                const int k = odd + (r.rev ? 15 - i : i);       // nibble of the 18 loaded
                const uint32_t byte = (k >> 1) < 8 ? (uint32_t)(w >> (8 * (k >> 1))) & 0xFFu : x;
                const uint32_t nib = (k & 1) ? (byte & 15u) : (byte >> 4);
                const uint64_t c = ((nib < 8 ? lo : hi) >> (8 * (nib & 7))) & 0xFFull;
                v[i >> 3] |= c << (8 * (i & 7));
            }
            return;
        }
        const int64_t q0 = k0 - (5 + r.L + r.S);       // quality index
        if (q0 >= 0 && q0 + 16 <= r.S) {
            if (r.no_qual) {
                v[0] = v[1] = 0x2222222222222222ull;
            } else if (!r.rev) {
                v[0] = cnq_phred8(cnq_load8(r.qual + q0));
                v[1] = cnq_phred8(cnq_load8(r.qual + q0 + 8));
            } else {
                v[1] = cnq_phred8(cnq_bswap8(cnq_load8(r.qual + (r.S - 16 - q0))));
                v[0] = cnq_phred8(cnq_bswap8(cnq_load8(r.qual + (r.S - 8 - q0))));
            }
            return;
        }
    }
    int64_t o1 = A.out[ri + 1];
    uint64_t v0 = 0, v1 = 0;
    for (int j = 0; j < m; ++j) {
        const int64_t q = p + j;
        if (q >= o1) {                      // (q < out[n]: there is a record with text behind this one, inside [ri + 1, r1])
            ri = cnq_find(A.out, ri + 1, r1, q);
            r = cnq_rec(A.text + A.off[ri]);
            o = A.out[ri];
            o1 = A.out[ri + 1];
        }
        const uint64_t c = (uint64_t)cnq_byte(r, q - o) << (8 * (j & 7));
        if (j < 8) v0 |= c;
        else v1 |= c;
    }
    v[0] = v0;
    v[1] = v1;
}
