// bam.hpp — the BAM header, the record chain and the record / CIGAR walk behind cornetto_bamdepth_*() (include/cornetto_accel.h states
// the rules): ONE source for the device (bam.hip: a wave per record) and for the CPU (tools/sim/bam_sim.cc: the same statements with the 64
// lanes run one after the other, under the host sanitizers against the Python oracle; cli/host_backend.c's rules are the same, in C).
// What tells the two builds apart is the lane shim S (as in inflate.hpp):
//   S::first(), S::step()   the lanes this thread of control runs: {lane, 64} on the device, {0, 1} on the CPU
//   S::SLOTS, S::slot(l)    where lane l keeps a per-lane value: 0 on the device (a register), l on the CPU (an array of 64)
//   S::leader()             one lane of the wave
//   S::scan(v)              inclusive add-scan of the lanes' 64-bit values, in place
//   S::last(v)              lane 63's value, in every lane;  S::sum(v): the sum of the lanes' values, in every lane
// Bounds come from the code, never from the input: cnb_frame() returns records that lie wholly inside the text; cnb_record() reads inside
// [rec, rec + 4 + block_size) only — the fixed-field equation is checked before the CIGAR is touched, every auxiliary field against the
// record's end before it is read — and hands the sink positions inside [0, contig length] of a contig in [0, n_ref) only.
// Records are not aligned in the text: every field is put together from byte loads (cnb_u32), which need no alignment; the 64 lanes of a
// CIGAR batch read 256 consecutive bytes.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/cornetto_accel.h"

#if defined(__HIPCC__)
#define CNB_HD __host__ __device__
#else
#define CNB_HD
#endif

#define CNB_LANES(l) for (int l = S::first(); l < 64; l += S::step())

enum { CNB_OK = 0, CNB_SHORT = 1, CNB_TRUNC = 2, CNB_FIELDS = 3, CNB_REFID = 4, CNB_CG = 5, CNB_BGZF = 6 };   // cornetto_bamerr_t.kind

CNB_HD static inline uint32_t cnb_u32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
CNB_HD static inline uint32_t cnb_u16(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }

// ---- header (host) ----------------------------------------------------------------------------------------------------------------------
// magic, l_text, text, n_ref, then per contig l_name, name (NUL included), l_ref.  -> CORNETTO_OK, 1 (more bytes needed) or CORNETTO_E_FORMAT
static inline int cnb_header(const uint8_t *buf, int64_t n, int32_t *n_ref, char ***names, int32_t **lens, int64_t *header_bytes)
{
    static const uint8_t magic[4] = {'B', 'A', 'M', 1};
    for (int64_t i = 0; i < 4 && i < n; ++i)
        if (buf[i] != magic[i]) return CORNETTO_E_FORMAT;
    if (n < 8) return 1;
    const int32_t l_text = (int32_t)cnb_u32(buf + 4);
    if (l_text < 0) return CORNETTO_E_FORMAT;
    int64_t p = 8 + (int64_t)l_text;
    if (n - p < 4) return 1;
    const int32_t nr = (int32_t)cnb_u32(buf + p);
    if (nr < 0) return CORNETTO_E_FORMAT;
    p += 4;
    const int64_t first = p;
    for (int32_t i = 0; i < nr; ++i) {
        if (n - p < 4) return 1;
        const int32_t l_name = (int32_t)cnb_u32(buf + p);
        if (l_name < 1) return CORNETTO_E_FORMAT;
        p += 4;
        if (n - p < (int64_t)l_name + 4) return 1;
        p += l_name;
        if ((int32_t)cnb_u32(buf + p) < 0) return CORNETTO_E_FORMAT;
        p += 4;
    }
    char **nm = (char **)malloc((size_t)(nr > 0 ? nr : 1) * sizeof(char *));
    int32_t *ln = (int32_t *)malloc((size_t)(nr > 0 ? nr : 1) * sizeof(int32_t));
    if (!nm || !ln) { free(nm); free(ln); return CORNETTO_E_NOMEM; }
    int64_t q = first;
    for (int32_t i = 0; i < nr; ++i) {
        const int32_t l_name = (int32_t)cnb_u32(buf + q);
        q += 4;
        nm[i] = (char *)malloc((size_t)l_name + 1);
        if (!nm[i]) {
            for (int32_t k = 0; k < i; ++k) free(nm[k]);
            free(nm); free(ln);
            return CORNETTO_E_NOMEM;
        }
        memcpy(nm[i], buf + q, (size_t)l_name);
        nm[i][l_name] = 0;          // (the name ends at its first NUL: l_name counts one)
        q += l_name;
        ln[i] = (int32_t)cnb_u32(buf + q);
        q += 4;
    }
    *n_ref = nr;
    *names = nm;
    *lens = ln;
    *header_bytes = p;
    return CORNETTO_OK;
}

// ---- the record chain -------------------------------------------------------------------------------------------------------------------
// Follows block_size, block_size, ... from `at`: the offsets of the records that lie wholly inside text[0 .. n) -> off[0 .. cap), their
// number returned; *end: the first byte that belongs to no returned record; *err: CNB_SHORT when the walk met a block_size (*err_a) below 32
// there.  cap >= (n - at) / 36 + 1 holds every record there can be.
CNB_HD static inline int64_t cnb_frame(const uint8_t *text, int64_t at, int64_t n, uint32_t *off, int64_t cap, int64_t *end, int32_t *err, int32_t *err_a)
{
    int64_t k = 0;
    *err = CNB_OK;
    *err_a = 0;
    while (k < cap && n - at >= 4) {
        const int32_t bs = (int32_t)cnb_u32(text + at);
        if (bs < 32) {
            *err = CNB_SHORT;
            *err_a = bs;
            break;
        }
        if ((int64_t)bs > n - at - 4) break;      // the record goes on behind the text
        off[k++] = (uint32_t)at;
        at += 4 + (int64_t)bs;
    }
    *end = at;
    return k;
}

// ---- one record -------------------------------------------------------------------------------------------------------------------------
struct CnbOut {
    int32_t ref_id, pos, mapq, flag, counted, n_ops;
    int64_t span, bases;
};
struct CnbErr {
    int32_t kind, a, b;
};
struct CnbRefs {
    int32_t n_ref;
    const int32_t *len;   // [n_ref]
    const int64_t *off;   // [n_ref] element of the difference arrays where the contig starts
};

CNB_HD static inline int32_t cnb_cap31(int64_t v) { return v > 0x7fffffffll ? 0x7fffffff : (int32_t)v; }

// The CG:B,I array among the auxiliary fields data[p .. bs) -> 1: found (*cig, *n_ops), 0: none (fields that do not parse end the search:
// no tag), -1: it runs past the record (*a elements, *b bytes of room).  Wave-uniform: every lane walks the same fields.
CNB_HD static inline int cnb_find_cg(const uint8_t *data, int64_t p, int64_t bs, const uint8_t **cig, int64_t *n_ops, int32_t *a, int32_t *b)
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
            if (t0 == 'C' && t1 == 'G' && sub == 'I') {
                if (cnt * 4 > bs - p) {
                    *a = cnb_cap31(cnt);
                    *b = (int32_t)(bs - p);
                    return -1;
                }
                *cig = data + p;
                *n_ops = cnt;
                return 1;
            }
            sz = cnt * es;
        } else return 0;
        if (sz > bs - p) return 0;
        p += sz;
    }
    return 0;
}

// rec: the record's block_size field, the record wholly readable (cnb_frame).  The checks, then — for a record that counts — the walk:
// sink.add(element, delta, mq) with mq = the record also counts in the second track.  A record of span bases from pos covers
// [pos, pos + span) except its D and N operations: +1 / -1 at the two ends of the record, -1 / +1 at the two ends of every D or N, each
// position cut to [0, length] (a pair that meets there is not issued).  That is one pair per run of M = X operations: what lies between two
// runs is a D or an N (two of those side by side issue a pair that cancels), and an I, S, H or P issues nothing.
template <class S, class Sink>
CNB_HD static inline int cnb_record(const uint8_t *rec, const CnbRefs &R, int32_t min_mapq, uint32_t skip_flags, Sink &sink, CnbOut &o, CnbErr &e)
{
    const int64_t bs = (int64_t)(int32_t)cnb_u32(rec);
    const uint8_t *data = rec + 4;
    o.ref_id = (int32_t)cnb_u32(data);
    o.pos = (int32_t)cnb_u32(data + 4);
    const int64_t l_read_name = data[8];
    o.mapq = data[9];
    const int64_t n_cigar = cnb_u16(data + 12);
    o.flag = (int32_t)cnb_u16(data + 14);
    const int64_t l_seq = (int64_t)cnb_u32(data + 16);
    o.counted = 0;
    o.n_ops = 0;
    o.span = o.bases = 0;
    e.kind = CNB_OK;
    e.a = e.b = 0;
    const int64_t fixed = 32 + l_read_name + 4 * n_cigar + (l_seq + 1) / 2 + l_seq;
    if (fixed > bs) {
        e.kind = CNB_FIELDS;
        e.a = cnb_cap31(fixed);
        e.b = (int32_t)bs;
        return e.kind;
    }
    if (o.ref_id < -1 || o.ref_id >= R.n_ref) {
        e.kind = CNB_REFID;
        e.a = o.ref_id;
        e.b = R.n_ref;
        return e.kind;
    }
    if (o.ref_id < 0 || ((uint32_t)o.flag & skip_flags) != 0) return CNB_OK;
    const uint8_t *cig = data + 32 + l_read_name;
    int64_t n_ops = n_cigar;
    if (n_cigar == 2) {
        const uint32_t op0 = cnb_u32(cig), op1 = cnb_u32(cig + 4);
        if ((op0 & 15u) == 4u && (int64_t)(op0 >> 4) == l_seq && (op1 & 15u) == 3u) {
            if (cnb_find_cg(data, fixed, bs, &cig, &n_ops, &e.a, &e.b) < 0) {
                e.kind = CNB_CG;
                return e.kind;
            }
        }
    }
    o.counted = 1;
    o.n_ops = cnb_cap31(n_ops);
    const bool mq = o.mapq >= min_mapq;
    const int64_t len = R.len[o.ref_id], off = R.off[o.ref_id], pos = o.pos;
    int64_t carry = 0, gone = 0;      // reference bases in front of the batch; D / N bases inside the contig
    for (int64_t base = 0; base < n_ops; base += 64) {
        unsigned long long adv[S::SLOTS];
        unsigned long long cut[S::SLOTS];
        CNB_LANES(l)
        {
            const int64_t i = base + l;
            const uint32_t op = i < n_ops ? cnb_u32(cig + 4 * i) : 0u;
            const uint32_t k = op & 15u;
            adv[S::slot(l)] = (k == 0u || k == 2u || k == 3u || k == 7u || k == 8u) ? (unsigned long long)(op >> 4) : 0ull;
            cut[S::slot(l)] = (k == 2u || k == 3u) ? 1ull : 0ull;
        }
        unsigned long long inc[S::SLOTS];
        CNB_LANES(l) inc[S::slot(l)] = adv[S::slot(l)];
        S::scan(inc);
        CNB_LANES(l)
        {
            unsigned long long g = 0;
            if (cut[S::slot(l)] && adv[S::slot(l)]) {
                int64_t en = pos + carry + (int64_t)inc[S::slot(l)], st = en - (int64_t)adv[S::slot(l)];
                st = st < 0 ? 0 : (st > len ? len : st);
                en = en < 0 ? 0 : (en > len ? len : en);
                if (st < en) {
                    sink.add(off + st, -1, mq);
                    sink.add(off + en, 1, mq);
                    g = (unsigned long long)(en - st);
                }
            }
            cut[S::slot(l)] = g;
        }
        carry += (int64_t)S::last(inc);
        gone += (int64_t)S::sum(cut);
    }
    int64_t st = pos, en = pos + carry;
    st = st < 0 ? 0 : (st > len ? len : st);
    en = en < 0 ? 0 : (en > len ? len : en);
    if (st < en && S::leader()) {
        sink.add(off + st, 1, mq);
        sink.add(off + en, -1, mq);
    }
    o.span = carry;
    o.bases = (st < en ? en - st : 0) - gone;
    return CNB_OK;
}
