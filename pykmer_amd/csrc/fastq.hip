// fastq.hip -- the FASTQ front end of the indexer for gfx950.
//
// A FASTQ feed is turned, on the device, into the FASTA text it stands for (README "FASTQ input"): line roles are
// line numbers mod 4 counted from the start of the stream; line 1 ('@' -> '>') and line 2 are kept with their
// terminators, lines 3 and 4 are dropped, and so are the terminators of empty header lines and of the empty sequence
// lines behind them (the blank lines after the last record).  The result goes through the FASTA pipeline unchanged.
//
// Same plan as the structure pass (fasta_fsm.h): the bytes are cut into 64-byte lane pieces, 256 pieces per 16 KiB
// chunk.  A piece's summary is what it does to the stream state -- terminators, kept bytes for each of the 4 roles it
// may be entered in, the length and blankness of its last open line -- and summaries compose associatively:
//   k_fq_count  one summary per chunk
//   k_fq_scan   one workgroup: the exact state at every chunk, seeded by the carry; the carry moves to the feed's end
//   k_fq_write  every lane re-derives its own state, copies its kept bytes (compacted in LDS, written as dwords), checks
//               the bytes at its line starts and writes the per-record header offsets and line 2 / line 4 lengths
//   k_fq_check  line 2 against line 4 of every record whose line 4 ended in this feed
//   k_fq_write_held  k_fq_write for base qualities: behind text held back from earlier feeds, and noting where line 2 went
//   k_fq_mask   base qualities only (threshold byte tq > 0): every line-4 byte below tq turns its line-2 byte in the emitted
//               text into 'N'; the text of a record whose line 4 is still open stays at the front of out[] (`held` bytes)
// Nothing waits for the host: errors, the need for a larger record array and the new totals sit in FqCarry, which the
// host reads with the feed's own read-back.
#include "fasta_fsm.h"
#include "pk_kernels.h"

namespace pk {

namespace {

typedef unsigned __int128 u128;

// x[i & 3] by selects: an indexed register array would live in scratch
template <class T> __device__ __forceinline__ T pick4(const T (&x)[4], uint32_t i) {
    i &= 3u;
    return i == 0u ? x[0] : i == 1u ? x[1] : i == 2u ? x[2] : x[3];
}

__device__ __forceinline__ FqSum fq_identity() {
    FqSum z;
    z.nt = 0; z.tail = 0; z.kept[0] = z.kept[1] = z.kept[2] = z.kept[3] = 0; z.ws = 1; z.pad = 0;
    return z;
}
__device__ __forceinline__ FqSum fq_compose(const FqSum &a, const FqSum &b) {   // a first, then b
    FqSum c;
    c.nt = a.nt + b.nt;
#pragma unroll
    for (uint32_t r = 0; r < 4; r++) c.kept[r] = a.kept[r] + pick4(b.kept, r + a.nt);
    c.tail = b.nt ? b.tail : a.tail + b.tail;
    c.ws = b.nt ? b.ws : (a.ws & b.ws);
    c.pad = 0;
    return c;
}
__device__ __forceinline__ FqState fq_apply(const FqState &s, const FqSum &x) {
    FqState o;
    o.line = s.line + x.nt;
    o.out = s.out + pick4(x.kept, (uint32_t)s.line);
    o.curlen = x.nt ? (uint64_t)x.tail : s.curlen + x.tail;
    o.ws = x.nt ? x.ws : (s.ws & x.ws);
    o.pad = 0;
    return o;
}

// Per-byte class masks of one lane piece, bit i <-> byte i.  Lookback masks are built on 68 bits: bit i + 4 <-> byte i,
// i = -4 .. 63; bytes before the start of the stream read as '\n' (a line starts at byte 0).
struct FqMasks {
    unsigned long long ts;        // terminator starts: '\r', or '\n' not after '\r'
    unsigned long long cont;      // the '\n' of a "\r\n" pair (belongs to the line the '\r' ended)
    unsigned long long tb;        // terminator bytes
    unsigned long long ls;        // line starts
    unsigned long long nws;       // neither terminator nor str.strip() whitespace
    unsigned long long dropa;     // terminator bytes of empty lines (dropped if the line is a header line)
    unsigned long long dropb;     // ... of an empty line behind an empty line (dropped if it is a sequence line)
    unsigned long long cls[4];    // bytes of the lines 0, 1, 2, 3 mod 4 after the piece's entry line
    uint32_t nb;
};

__device__ __forceinline__ uint32_t swar_eq(uint32_t w, uint32_t rep) { return swar_zero(w ^ rep); }

__device__ __forceinline__ void fq_masks(const uint8_t *mine, uint32_t nb, uint32_t prev4, FqMasks &m) {
    uint32_t cr[2] = {0, 0}, nl[2] = {0, 0}, ws[2] = {0, 0};
    const uint4 *quads = reinterpret_cast<const uint4 *>(mine);
#pragma unroll
    for (int q = 0; q < PIECE / 16; q++) {
        const uint4 v = quads[q];
        const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t w = w4[j];
            const int d = q * 4 + j;
            // str.strip() whitespace: 9..13, 28..31, 32
            const uint32_t wsb = (swar_less(w, 0x0e0e0e0eu) & ~swar_less(w, 0x09090909u)) |
                                 (swar_less(w, 0x20202020u) & ~swar_less(w, 0x1c1c1c1cu)) | swar_eq(w, 0x20202020u);
            cr[d >> 3] |= movemask4(swar_eq(w, 0x0d0d0d0du)) << (4 * (d & 7));
            nl[d >> 3] |= movemask4(swar_eq(w, 0x0a0a0a0au)) << (4 * (d & 7));
            ws[d >> 3] |= movemask4(wsb) << (4 * (d & 7));
        }
    }
    const unsigned long long in_range = nb >= 64u ? ~0ull : ((1ull << nb) - 1ull);
    uint32_t pcr = 0, pnl = 0;                                           // bytes -4 .. -1 -> bits 0 .. 3
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint32_t c = (prev4 >> (8 * j)) & 0xffu;
        pcr |= (c == 13u ? 1u : 0u) << j;
        pnl |= (c == 10u ? 1u : 0u) << j;
    }
    const unsigned long long CR = ((((unsigned long long)cr[1]) << 32) | cr[0]) & in_range;
    const unsigned long long NL = ((((unsigned long long)nl[1]) << 32) | nl[0]) & in_range;
    const unsigned long long WS = ((((unsigned long long)ws[1]) << 32) | ws[0]) & in_range;
    const u128 XCR = ((u128)CR << 4) | pcr, XNL = ((u128)NL << 4) | pnl;
    const u128 XTB = XCR | XNL;
    const u128 XTS = XCR | (XNL & ~(XCR << 1));
    const u128 XCONT = XNL & (XCR << 1);
    const u128 XE = XTS & (XTB << 1);                                    // the line ending here is empty
    const u128 XEP = ((XCONT << 1) & (XTB << 3)) | (~(XCONT << 1) & (XTB << 2));   // ... and so is the line before it
    const u128 XA = XTS & XE, XB = XTS & XE & XEP;
    const u128 DA = XA | ((XA << 1) & XCONT), DB = XB | ((XB << 1) & XCONT);
    m.ts = (unsigned long long)(XTS >> 4);
    m.cont = (unsigned long long)(XCONT >> 4);
    m.tb = CR | NL;
    m.ls = (unsigned long long)((XTB << 1) >> 4) & ~m.cont & in_range;
    m.nws = ~WS & in_range;
    m.dropa = (unsigned long long)(DA >> 4);
    m.dropb = (unsigned long long)(DB >> 4);
    m.nb = nb;
    // classes: a line runs from behind one terminator up to and including the next one (its "\r\n" partner too)
    const unsigned long long cont0 = m.cont & 1ull;
    unsigned long long c0 = 0, c1 = 0, c2 = 0, c3 = cont0;               // cont0: the end of a line that began before the piece
    unsigned long long rest = in_range & ~cont0, t = m.ts;
    uint32_t j = 0;
    auto add = [&](unsigned long long bits) {
        const uint32_t q = j & 3u;
        c0 |= q == 0u ? bits : 0ull; c1 |= q == 1u ? bits : 0ull; c2 |= q == 2u ? bits : 0ull; c3 |= q == 3u ? bits : 0ull;
    };
    while (t) {
        const uint32_t p = (uint32_t)__builtin_ctzll(t);
        const uint32_t e = p + (p < 63u ? (uint32_t)((m.cont >> (p + 1u)) & 1ull) : 0u);   // last byte of the terminator
        const unsigned long long upto = e >= 63u ? ~0ull : ((1ull << (e + 1u)) - 1ull);
        add(rest & upto);
        rest &= ~upto;
        t &= t - 1ull;
        j++;
    }
    add(rest);
    m.cls[0] = c0; m.cls[1] = c1; m.cls[2] = c2; m.cls[3] = c3;
}

// bytes kept when the piece is entered in role r
__device__ __forceinline__ unsigned long long fq_kept(const FqMasks &m, uint32_t r) {
    return (pick4(m.cls, 4u - r) & ~m.dropa) | (pick4(m.cls, 5u - r) & ~m.dropb);
}

__device__ __forceinline__ FqSum fq_sum_of(const FqMasks &m) {
    FqSum s;
    s.nt = (uint32_t)__popcll(m.ts);
#pragma unroll
    for (uint32_t r = 0; r < 4; r++) s.kept[r] = (uint32_t)__popcll(fq_kept(m, r));
    const unsigned long long in_range = m.nb >= 64u ? ~0ull : ((1ull << m.nb) - 1ull);
    unsigned long long open;                                             // bytes of the line left open at the end
    if (m.ts) {
        const uint32_t p = 63u - (uint32_t)__builtin_clzll(m.ts);
        const uint32_t e = p + (p < 63u ? (uint32_t)((m.cont >> (p + 1u)) & 1ull) : 0u);
        open = e >= 63u ? 0ull : (in_range & ~((1ull << (e + 1u)) - 1ull));
    } else {
        open = in_range & ~(m.cont & 1ull);
    }
    s.tail = (uint32_t)__popcll(open);
    s.ws = (open & m.nws) ? 0u : 1u;
    s.pad = 0;
    return s;
}

// Exclusive scan of the 256 lane summaries of a workgroup (sh: 2 x 256 FqSum of LDS); returns the lane's prefix, *total
// the workgroup's summary.
__device__ __forceinline__ FqSum fq_wg_scan(const FqSum &mine, FqSum *sh, FqSum *total) {
    const uint32_t t = threadIdx.x;
    sh[t] = mine;
    __syncthreads();
    uint32_t cur = 0;
#pragma unroll 1
    for (uint32_t d = 1; d < (uint32_t)WG; d <<= 1) {
        FqSum v = sh[cur * WG + t];
        if (t >= d) v = fq_compose(sh[cur * WG + t - d], v);
        sh[(cur ^ 1u) * WG + t] = v;
        cur ^= 1u;
        __syncthreads();
    }
    *total = sh[cur * WG + WG - 1];
    const FqSum ex = t ? sh[cur * WG + t - 1] : fq_identity();
    __syncthreads();
    return ex;
}

// the 4 bytes in front of lane piece `lane` of chunk `chunk` (byte -1 highest)
__device__ __forceinline__ uint32_t fq_prev4(const uint8_t *__restrict__ f, uint32_t chunk, const uint8_t *lds, uint32_t prev4_feed) {
    const uint32_t lane = threadIdx.x;
    if (lane) return *reinterpret_cast<const uint32_t *>(lds + (lane - 1u) * LDS_STRIDE + 60u);
    if (chunk) return *reinterpret_cast<const uint32_t *>(f + (uint64_t)chunk * CHUNK - 4u);
    return prev4_feed;
}

__global__ __launch_bounds__(WG) void k_fq_count(const uint8_t *__restrict__ f, uint64_t n, const FqCarry *__restrict__ carry,
                                                 FqSum *__restrict__ sums) {
    __shared__ __align__(16) uint8_t lds[WG * LDS_STRIDE];
    __shared__ FqSum sh[2 * WG];
    const uint32_t chunk = blockIdx.x;
    const uint64_t base = (uint64_t)chunk * CHUNK;
    stage_chunk(f, base, n, lds);
    __syncthreads();
    const uint8_t *mine = lds + threadIdx.x * LDS_STRIDE;
    FqMasks m;
    fq_masks(mine, piece_len(base, n), fq_prev4(f, chunk, lds, carry->prev4), m);
    FqSum tot;
    fq_wg_scan(fq_sum_of(m), sh, &tot);
    if (threadIdx.x == 0) sums[chunk] = sh[WG - 1];                      // = tot: the scan ends in the first half (8 steps)
}

// One workgroup: every thread composes a run of consecutive chunks, the runs are scanned, then every thread walks its
// run again from its exact state.  The carry moves to the end of the feed; the state at its start stays in `in`.
constexpr uint32_t SCAN_T = 1024;
__global__ __launch_bounds__(SCAN_T) void k_fq_scan(const uint8_t *__restrict__ f, uint64_t n, const FqSum *__restrict__ sums,
                                                    uint32_t n_chunks, FqState *__restrict__ st, uint32_t tq, FqCarry *__restrict__ carry) {
    __shared__ FqSum sh[2 * SCAN_T];
    const uint32_t t = threadIdx.x;
    const uint32_t per = (n_chunks + SCAN_T - 1) / SCAN_T;
    const uint32_t lo = min(n_chunks, t * per), hi = min(n_chunks, lo + per);
    FqSum acc = fq_identity();
    for (uint32_t c = lo; c < hi; c++) acc = fq_compose(acc, sums[c]);
    sh[t] = acc;
    __syncthreads();
    uint32_t cur = 0;
    for (uint32_t d = 1; d < SCAN_T; d <<= 1) {
        FqSum v = sh[cur * SCAN_T + t];
        if (t >= d) v = fq_compose(sh[cur * SCAN_T + t - d], v);
        sh[(cur ^ 1u) * SCAN_T + t] = v;
        cur ^= 1u;
        __syncthreads();
    }
    const FqState s0 = carry->st;
    FqState s = t ? fq_apply(s0, sh[cur * SCAN_T + t - 1]) : s0;
    for (uint32_t c = lo; c < hi; c++) {
        st[c] = s;
        s = fq_apply(s, sums[c]);
    }
    __syncthreads();                                                     // every thread has read carry->st
    if (t == SCAN_T - 1) {
        FqCarry &cy = *carry;
        cy.in = s0;
        cy.prev4_in = cy.prev4;
        cy.st = s;                                                       // the last thread's run ends the feed
        uint32_t p = cy.prev4;
        const uint64_t from = n > 4u ? n - 4u : 0u;
        for (uint64_t i = from; i < n; i++) p = (p >> 8) | ((uint32_t)f[i] << 24);
        cy.prev4 = p;
        cy.in_bytes = cy.bytes_fed;
        cy.bytes_fed += n;
        const uint64_t need = s.line / 4u + 1u;                          // records that may get a slot (the open one too)
        if (need > cy.need) cy.need = need;
        if (tq) cy.masked_in = cy.masked;
    }
}

__device__ __forceinline__ void fq_error(FqCarry *carry, uint64_t rec, uint32_t rule) {
    atomicMin((unsigned long long *)&carry->err, (unsigned long long)((rec << 3) | rule));
}

// The body of k_fq_write.  MASK (base qualities, k_fq_write_held): out[] begins with `held` bytes of earlier text, out2[] takes
// per record the bytes emitted before its line 2, and the count of k_fq_mask restarts.  Without it held = 0 and out2 is not
// touched: the kernel is the one it was before base qualities.
template <bool MASK>
__device__ __forceinline__ void fq_write_body(const uint8_t *__restrict__ f, uint64_t n, const FqState *__restrict__ st,
                                              uint8_t *__restrict__ out, uint64_t held, FqRec *__restrict__ recs,
                                              uint64_t *__restrict__ out2, uint64_t recs_cap, FqCarry *__restrict__ carry) {
    __shared__ __align__(16) uint8_t lds[WG * LDS_STRIDE];
    __shared__ __align__(16) uint8_t obuf[CHUNK + 16];
    __shared__ FqSum sh[2 * WG];
    __shared__ unsigned long long last_full;
    const uint32_t chunk = blockIdx.x;
    const uint64_t base = (uint64_t)chunk * CHUNK;
    if (threadIdx.x == 0) last_full = 0;
    stage_chunk(f, base, n, lds);
    __syncthreads();
    const uint8_t *mine = lds + threadIdx.x * LDS_STRIDE;
    FqMasks m;
    const uint32_t nb = piece_len(base, n);
    fq_masks(mine, nb, fq_prev4(f, chunk, lds, carry->prev4_in), m);
    FqSum tot;
    const FqSum ex = fq_wg_scan(fq_sum_of(m), sh, &tot);
    const FqState c0 = st[chunk];
    const FqState s = fq_apply(c0, ex);
    const uint64_t out0 = carry->in.out - held;                         // out[] starts there: `held` bytes before this feed's text
    if (MASK && chunk == 0u && threadIdx.x == 0) carry->masked = carry->masked_in;   // k_fq_mask counts this feed from there, each time it runs
    const uint32_t r = (uint32_t)(s.line & 3u);
    const uint64_t g0 = carry->in_bytes + base + (uint64_t)threadIdx.x * PIECE;   // stream offset of the piece

    // ---- bytes: compacted into LDS at their place in the chunk's output, '@' -> '>' at the start of header lines
    const unsigned long long keep = fq_kept(m, r);
    const unsigned long long hdr_start = m.ls & pick4(m.cls, 4u - r);
    const uint32_t lead = (uint32_t)((c0.out - out0) & 3u);
    {
        uint32_t o = lead + (uint32_t)(s.out - c0.out);
        unsigned long long k = keep;
        while (k) {
            const uint32_t p = (uint32_t)__builtin_ctzll(k);
            obuf[o++] = ((hdr_start >> p) & 1ull) ? (uint8_t)'>' : mine[p];
            k &= k - 1ull;
        }
    }

    // ---- lines: checks at line starts, lengths at terminators, the header offset of every record
    {
        unsigned long long t = m.ts;
        uint64_t line = s.line;
        uint32_t a = (uint32_t)(m.cont & 1ull);                          // first byte of the current segment
        bool at_start = ((m.ls >> a) & 1ull) != 0ull;                   // the segment begins its line
        uint64_t len0 = s.curlen;                                        // bytes of its line before the piece
        bool ws_in = s.ws != 0u;
        unsigned long long full = 0;                                     // 1 + the last line with content
        for (;;) {
            const bool term = t != 0ull;
            const uint32_t p = term ? (uint32_t)__builtin_ctzll(t) : nb;   // the segment is bytes [a, p)
            const uint32_t role = (uint32_t)(line & 3u);
            const uint64_t rec = line >> 2;
            const unsigned long long seg = (p >= 64u ? ~0ull : ((1ull << p) - 1ull)) & ~((1ull << a) - 1ull);
            if (at_start) {
                len0 = 0; ws_in = true;
                const uint32_t c = a < nb ? mine[a] : 10u;               // a line start at the end of the feed: nothing yet
                if (a < nb) {
                    if (role == 0u) {
                        if (rec < recs_cap) recs[rec].line1 = g0 + a;
                        if (c == '\r' || c == '\n') {                    // an empty header line: only blank lines may follow
                            atomicMin((unsigned long long *)&carry->trail, (unsigned long long)line);
                        } else if (c != '@') {
                            fq_error(carry, rec, FQ_RULE_AT);
                        }
                    } else if (role == 2u && c != '+') {
                        fq_error(carry, rec, FQ_RULE_PLUS);
                    } else if (MASK && role == 1u && rec < recs_cap) {
                        out2[rec] = s.out + (uint32_t)__popcll(keep & ((1ull << a) - 1ull));
                    }
                }
            }
            if (role == 1u && ws_in) {
                const unsigned long long x = m.nws & seg;
                if (x) {
                    if (mine[__builtin_ctzll(x)] == '>') fq_error(carry, rec, FQ_RULE_GT);
                }
            }
            if (seg) full = line + 1u;
            if (!term) break;
            const uint64_t len = len0 + (p - a);
            if (rec < recs_cap) {
                if (role == 1u) recs[rec].len2 = len;
                else if (role == 3u) recs[rec].len4 = len;
            }
            t &= t - 1ull;
            line++;
            a = p + 1u + (p < 63u ? (uint32_t)((m.cont >> (p + 1u)) & 1ull) : 0u);
            if (a > 64u) a = 64u;
            at_start = a < 64u;                                          // else the line starts in the next piece
            if (a >= 64u) break;
            len0 = 0;
        }
        if (full) atomicMax(&last_full, full);
    }
    __syncthreads();
    if (threadIdx.x == 0 && last_full) atomicMax((unsigned long long *)&carry->full, last_full);

    // ---- the chunk's output [c0.out, c0.out + tot.kept[role]) as dwords; edge words byte by byte
    const uint64_t o_lo = c0.out - out0, o_hi = o_lo + pick4(tot.kept, (uint32_t)c0.line);
    const uint64_t w_lo = o_lo & ~3ull;
    for (uint64_t w = w_lo + 4u * threadIdx.x; w < o_hi; w += 4u * WG) {
        const uint32_t li = (uint32_t)(w - w_lo);
        if (w >= o_lo && w + 4u <= o_hi) {
            *reinterpret_cast<uint32_t *>(out + w) = *reinterpret_cast<const uint32_t *>(obuf + li);
        } else {
            for (uint32_t j = 0; j < 4u; j++)
                if (w + j >= o_lo && w + j < o_hi) out[w + j] = obuf[li + j];
        }
    }
}

__global__ __launch_bounds__(WG) void k_fq_write(const uint8_t *__restrict__ f, uint64_t n, const FqState *__restrict__ st,
                                                 uint8_t *__restrict__ out, FqRec *__restrict__ recs, uint64_t recs_cap,
                                                 FqCarry *__restrict__ carry) {
    fq_write_body<false>(f, n, st, out, 0u, recs, nullptr, recs_cap, carry);
}
__global__ __launch_bounds__(WG) void k_fq_write_held(const uint8_t *__restrict__ f, uint64_t n, const FqState *__restrict__ st,
                                                      uint8_t *__restrict__ out, uint64_t held, FqRec *__restrict__ recs,
                                                      uint64_t *__restrict__ out2, uint64_t recs_cap, FqCarry *__restrict__ carry) {
    fq_write_body<true>(f, n, st, out, held, recs, out2, recs_cap, carry);
}

// line 2 against line 4 of the records whose line 4 ended in this feed
__global__ __launch_bounds__(WG) void k_fq_check(const FqRec *__restrict__ recs, uint64_t recs_cap, FqCarry *__restrict__ carry) {
    const uint64_t lo = carry->in.line / 4u, hi = carry->st.line / 4u;
    for (uint64_t rec = lo + (uint64_t)blockIdx.x * WG + threadIdx.x; rec < hi && rec < recs_cap; rec += (uint64_t)gridDim.x * WG)
        if (recs[rec].len2 != recs[rec].len4) fq_error(carry, rec, FQ_RULE_LEN);
}

// str.strip() whitespace (9 .. 13, 28 .. 31, 32) among the bytes of a word -> 0x80 flags
__device__ __forceinline__ uint32_t swar_ws(uint32_t w) {
    return (swar_less(w, 0x0e0e0e0eu) & ~swar_less(w, 0x09090909u)) | (swar_less(w, 0x20202020u) & ~swar_less(w, 0x1c1c1c1cu)) |
           swar_eq(w, 0x20202020u);
}

// bytes of a word below tq (1 .. 255) as unsigned bytes -> 0x80 flags
__device__ __forceinline__ uint32_t swar_below(uint32_t w, uint32_t tq) {
    const uint32_t n7 = (tq > 0x80u ? tq - 0x80u : tq) * 0x01010101u;    // compared with the low 7 bits, 1 .. 0x80
    const uint32_t lt7 = ~(((w & 0x7f7f7f7fu) | 0x80808080u) - n7) & 0x80808080u;
    return tq > 0x80u ? ((~w & 0x80808080u) | (lt7 & w)) : (lt7 & ~w);
}

// Base qualities (README "Base quality"), behind k_fq_write of the same feed: byte o of record r's line 4 below tq turns
// byte o of r's line 2 in the emitted text into 'N', unless o >= len2[r] (a malformed record: k_fq_check reports it), the
// record has no slot (the front end runs again) or the text byte is a str.strip() blank.  out[] holds the emitted bytes
// [in.out - held, st.out): `held` bytes of records whose line 4 was still open, then this feed's text; out2[r] and
// len2[r] were written when line 2 went by, in this feed or an earlier one.  Every text byte has one quality byte, so no
// two lanes meet (a lane patches the text dwords that lie wholly under its bytes as words, the rest byte by byte), and a
// second run over the same feed finds the same bytes: the count restarts from masked_in (k_fq_write_held).
// The first thread also leaves the offset up to which the text is settled: the start of line 2 of the open record.
__global__ __launch_bounds__(WG) void k_fq_mask(const uint8_t *__restrict__ f, uint64_t n, const FqState *__restrict__ st,
                                                uint8_t *__restrict__ out, uint64_t held, const FqRec *__restrict__ recs,
                                                const uint64_t *__restrict__ out2, uint64_t recs_cap, uint32_t tq, FqCarry *__restrict__ carry) {
    __shared__ __align__(16) uint8_t lds[WG * LDS_STRIDE];
    __shared__ FqSum sh[2 * WG];
    __shared__ uint32_t wg_masked;
    const uint32_t chunk = blockIdx.x;
    const uint64_t base = (uint64_t)chunk * CHUNK;
    if (threadIdx.x == 0) wg_masked = 0;
    stage_chunk(f, base, n, lds);
    __syncthreads();
    const uint8_t *mine = lds + threadIdx.x * LDS_STRIDE;
    FqMasks m;
    const uint32_t nb = piece_len(base, n);
    fq_masks(mine, nb, fq_prev4(f, chunk, lds, carry->prev4_in), m);
    FqSum tot;
    const FqSum ex = fq_wg_scan(fq_sum_of(m), sh, &tot);
    const FqState s = fq_apply(st[chunk], ex);
    const uint64_t out_lo = carry->in.out - held, out_hi = carry->st.out;   // the emitted bytes out[] holds

    unsigned long long low = 0;                                          // bytes below tq
    {
        const uint4 *quads = reinterpret_cast<const uint4 *>(mine);
        uint32_t lo32[2] = {0, 0};
#pragma unroll
        for (int q = 0; q < PIECE / 16; q++) {
            const uint4 v = quads[q];
            const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int d = q * 4 + j;
                lo32[d >> 3] |= movemask4(swar_below(w4[j], tq)) << (4 * (d & 7));
            }
        }
        low = ((((unsigned long long)lo32[1]) << 32) | lo32[0]) & (nb >= 64u ? ~0ull : ((1ull << nb) - 1ull));
    }

    uint32_t masked = 0;
    {   // the lines of the piece as k_fq_write walks them
        unsigned long long t = m.ts;
        uint64_t line = s.line;
        uint32_t a = (uint32_t)(m.cont & 1ull);
        uint64_t len0 = ((m.ls >> a) & 1ull) ? 0u : s.curlen;            // bytes of the segment's line before the piece
        for (;;) {
            const bool term = t != 0ull;
            const uint32_t p = term ? (uint32_t)__builtin_ctzll(t) : nb;   // the segment is bytes [a, p)
            const uint64_t rec = line >> 2;
            unsigned long long x = (p >= 64u ? ~0ull : ((1ull << p) - 1ull)) & ~((1ull << a) - 1ull) & low;
            if ((line & 3u) == 3u && x && rec < recs_cap) {
                const uint64_t len2 = recs[rec].len2, at = out2[rec] + len0;   // `at`: where the text byte of piece byte a lies
                const uint64_t room = len2 > len0 ? len2 - len0 : 0u;           // line-2 bytes from there on
                const uint32_t pe = (uint64_t)(p - a) <= room ? p : a + (uint32_t)room;   // piece bytes [a, pe) have a text byte
                x &= pe >= 64u ? ~0ull : ((1ull << pe) - 1ull);
                if (x && at >= out_lo && at + (pe - a) <= out_hi) {
                    const uint64_t t0 = at - out_lo - a;                        // out[t0 + i] is the text byte of piece byte i (t0 + a >= 0)
                    // the text dwords that lie inside [a, pe) are this lane's alone: read together, patched, written back
                    const uint32_t i_lo = a + (uint32_t)((0u - (t0 + a)) & 3u);
                    const uint32_t n_words = i_lo < pe ? (pe - i_lo) >> 2 : 0u;
                    uint32_t wv[PIECE / 4];
#pragma unroll
                    for (int j = 0; j < PIECE / 4; j++) {
                        const uint32_t i = i_lo + 4u * j;
                        const uint32_t bits = (uint32_t)j < n_words ? (uint32_t)(x >> (i & 63u)) & 15u : 0u;
                        wv[j] = bits ? *reinterpret_cast<const uint32_t *>(out + (t0 + i)) : 0u;
                    }
#pragma unroll
                    for (int j = 0; j < PIECE / 4; j++) {
                        const uint32_t i = i_lo + 4u * j;
                        const uint32_t bits = (uint32_t)j < n_words ? (uint32_t)(x >> (i & 63u)) & 15u : 0u;
                        if (bits) {
                            const uint32_t hit = ((bits * 0x00204081u) & 0x01010101u) & ~(swar_ws(wv[j]) >> 7);   // 0x01 per byte to replace
                            const uint32_t bytes = hit * 0xffu;
                            if (hit) *reinterpret_cast<uint32_t *>(out + (t0 + i)) = (wv[j] & ~bytes) | (0x4e4e4e4eu & bytes);
                            masked += (uint32_t)__popc(hit);
                        }
                    }
                    // the bytes in front of and behind those words share theirs with other lanes: byte by byte
                    const uint32_t i_hi = i_lo + 4u * n_words;
                    if (n_words) x &= ((1ull << i_lo) - 1ull) | (i_hi >= 64u ? 0ull : ~((1ull << i_hi) - 1ull));
                    while (x) {
                        const uint32_t i = (uint32_t)__builtin_ctzll(x);
                        x &= x - 1ull;
                        if (!is_ws(out[t0 + i])) {
                            out[t0 + i] = (uint8_t)'N';
                            masked++;
                        }
                    }
                }
            }
            if (!term) break;
            t &= t - 1ull;
            line++;
            a = p + 1u + (p < 63u ? (uint32_t)((m.cont >> (p + 1u)) & 1ull) : 0u);
            if (a >= 64u) break;
            len0 = 0;
        }
    }
    if (masked) atomicAdd(&wg_masked, masked);
    __syncthreads();
    if (threadIdx.x == 0 && wg_masked) atomicAdd((unsigned long long *)&carry->masked, (unsigned long long)wg_masked);

    if (chunk == 0u && threadIdx.x == 0) {
        const FqState e = carry->st;
        const uint32_t role = (uint32_t)(e.line & 3u);
        const uint64_t rec = e.line >> 2;
        uint64_t settled = e.out;                                        // no line 2 is waiting for its line 4
        if (role >= 2u || (role == 1u && e.curlen > 0u)) settled = rec < recs_cap ? out2[rec] : out_lo;
        carry->settled = settled;
    }
}

}  // namespace

void launch_fq_front(const uint8_t *f, uint64_t n, FqSum *sums, FqState *st, uint8_t *out, uint64_t held, FqRec *recs, uint64_t *out2,
                     uint64_t recs_cap, uint32_t tq, FqCarry *carry, hipStream_t s) {
    const uint32_t n_chunks = (uint32_t)((n + CHUNK - 1) / CHUNK);
    hipLaunchKernelGGL(k_fq_count, dim3(n_chunks), dim3(WG), 0, s, f, n, (const FqCarry *)carry, sums);
    hipLaunchKernelGGL(k_fq_scan, dim3(1), dim3(SCAN_T), 0, s, f, n, (const FqSum *)sums, n_chunks, st, tq, carry);
    launch_fq_write(f, n, st, out, held, recs, out2, recs_cap, tq, carry, s);
}

void launch_fq_write(const uint8_t *f, uint64_t n, const FqState *st, uint8_t *out, uint64_t held, FqRec *recs, uint64_t *out2,
                     uint64_t recs_cap, uint32_t tq, FqCarry *carry, hipStream_t s) {
    const uint32_t n_chunks = (uint32_t)((n + CHUNK - 1) / CHUNK);
    if (tq) hipLaunchKernelGGL(k_fq_write_held, dim3(n_chunks), dim3(WG), 0, s, f, n, st, out, held, recs, out2, recs_cap, carry);
    else hipLaunchKernelGGL(k_fq_write, dim3(n_chunks), dim3(WG), 0, s, f, n, st, out, recs, recs_cap, carry);
    hipLaunchKernelGGL(k_fq_check, dim3(256), dim3(WG), 0, s, (const FqRec *)recs, recs_cap, carry);
    if (tq) hipLaunchKernelGGL(k_fq_mask, dim3(n_chunks), dim3(WG), 0, s, f, n, st, out, held, (const FqRec *)recs, (const uint64_t *)out2, recs_cap, tq, carry);
}

}  // namespace pk
