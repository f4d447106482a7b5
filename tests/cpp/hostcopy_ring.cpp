/* hostcopy_ring.cpp -- csrc/mm_hostcopy_plan.h on the host, a stand-alone program (tests/test_hostcopy_host.py builds it with
 * -fsanitize=thread and with -fsanitize=address,undefined and asserts the counts it prints).
 *
 *   plan      every len in {1 .. 3*4096+1} u {8 MiB - 4097 .. 8 MiB} x T in 1 .. 8: the slices with a < len tile [0, len) in
 *             order without overlap, every interior boundary a multiple of 4096, none empty; the chunks of seven byte counts
 *             tile [0, bytes); the direct / staged decision at 4 MiB - 1 and 4 MiB x cpus 1, 2 x pinned or not; the constants.
 *   budget    cpus 1 .. 256 x k = 1 .. 16 copies entering together (active = 1 .. k): with n = clamp(cpus / 2, 1, 8) copy a takes
 *             max(1, floor(n / a)) threads, and their sum is  sum_{j = 1 .. n} min(min(k, n), floor(n / j)) + max(0, k - n)
 *             (the lattice points under the hyperbola a j <= n, counted by rows instead of columns, and one thread for every
 *             copy past the n-th); for n = 8 the sums are 8 12 14 16 17 18 19 20 21 .. 28.  The first copy alone takes the
 *             whole n, so from k = 2 on the sum exceeds n: the copies do not share one budget of n.
 *   protocol  mm_hostcopy_ring over a fake transport whose "device" is a host array with a position-dependent pattern and whose
 *             slots are malloc'ed; issue records (off, len) and a pseudo-random number (0 .. 7) of "not ready" answers, query
 *             makes the memcpy into the slot at the moment it first answers "done".  A slot handed out before every worker has
 *             left it is then a write racing the workers' reads, a publish without release ordering a race too: the thread
 *             sanitizer reports both.  Chunk 64 KiB, 13 byte counts x T in {1, 2, 3, 5, 8} x destination offsets {0, 4, 60}
 *             into a buffer prefilled with 0x5a: status, every byte, and the bytes on both sides of the destination.  Then four
 *             cases with the library's own 8 MiB chunk.
 *   failures  issue fails at chunk j in {0, 3, 4, last}; query fails at the same j; the thread-start callable throws at thread
 *             0 and T - 1: the error (or "not started") comes back, every started thread is joined (the program ends), every
 *             byte of a published chunk is the source's or untouched, everything else still 0x5a. */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>

#include "../../mini_mcmc_amd/csrc/mm_hostcopy_plan.h"

static long g_failed = 0;

#define CHECK(cond, ...)                                                                                                           \
    do {                                                                                                                           \
        if (!(cond)) {                                                                                                             \
            if (++g_failed <= 20) {                                                                                                \
                std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond);                                                       \
                std::printf(__VA_ARGS__);                                                                                          \
                std::printf("\n");                                                                                                 \
            }                                                                                                                      \
        }                                                                                                                          \
    } while (0)

static unsigned char pattern(size_t i) { return (unsigned char)((i * 2654435761u >> 7) ^ (i >> 16) ^ 0x3c); }

/* ---- plan ---- */

static void check_slices(size_t len, int T)
{
    size_t next = 0;
    for (int t = 0; t < T; ++t) {
        const mm_hostcopy_slice s = mm_hostcopy_slice_of(len, T, t);
        if (s.a >= len)
            continue;
        CHECK(s.a == next, "len %zu T %d t %d: a %zu after %zu", len, T, t, s.a, next);
        CHECK(s.b > s.a && s.b <= len, "len %zu T %d t %d: [%zu, %zu)", len, T, t, s.a, s.b);
        CHECK(s.a % 4096 == 0 && (s.b == len || s.b % 4096 == 0), "len %zu T %d t %d: [%zu, %zu)", len, T, t, s.a, s.b);
        next = s.b;
    }
    CHECK(next == len, "len %zu T %d: covered %zu", len, T, next);
}

static long plan_slices()
{
    long n = 0;
    for (int T = 1; T <= 8; ++T) {
        for (size_t len = 1; len <= 3 * 4096 + 1; ++len, ++n)
            check_slices(len, T);
        for (size_t len = kHostcopyChunk - 4097; len <= kHostcopyChunk; ++len, ++n)
            check_slices(len, T);
    }
    return n;
}

static long plan_chunks()
{
    const size_t C = kHostcopyChunk;
    const size_t counts[] = {1, C - 1, C, C + 1, 4 * C, 4 * C + 1, 9 * C + 8191};
    long n = 0;
    for (size_t bytes : counts) {
        const size_t nc = mm_hostcopy_chunks(bytes, C);
        size_t next = 0;
        for (size_t i = 0; i < nc; ++i) {
            const mm_hostcopy_span c = mm_hostcopy_chunk(bytes, C, i);
            CHECK(c.off == next && c.len >= 1 && c.len <= C, "bytes %zu chunk %zu: off %zu len %zu", bytes, i, c.off, c.len);
            CHECK(i + 1 == nc || c.len == C, "bytes %zu chunk %zu: a short chunk before the last", bytes, i);
            next = c.off + c.len;
        }
        CHECK(next == bytes && nc == (bytes - 1) / C + 1, "bytes %zu: %zu chunks cover %zu", bytes, nc, next);
        ++n;
    }
    return n;
}

static long plan_decisions()
{
    static_assert(kHostcopyChunk == (size_t)8 << 20 && kHostcopyRing == 4 && kHostcopyDirectBelow == (size_t)4 << 20, "constants");
    long n = 0;
    const size_t M4 = (size_t)4 << 20;
    for (size_t bytes : {M4 - 1, M4})
        for (int cpus : {1, 2})
            for (bool pinned : {false, true}) {
                const bool staged = bytes == M4 && cpus == 2 && !pinned;
                CHECK(mm_hostcopy_direct(bytes, cpus, pinned) == !staged, "bytes %zu cpus %d pinned %d", bytes, cpus, (int)pinned);
                ++n;
            }
    return n;
}

/* ---- budget ---- */

static long budget()
{
    static const int sums8[16] = {8, 12, 14, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28};
    long cases = 0;
    for (int cpus = 1; cpus <= 256; ++cpus) {
        const int n = cpus / 2 < 1 ? 1 : cpus / 2 > 8 ? 8 : cpus / 2;
        for (int k = 1; k <= 16; ++k, ++cases) {
            int sum = 0;
            for (int a = 1; a <= k; ++a) {
                const int T = mm_hostcopy_threads(cpus, a);
                CHECK(T == (n / a > 1 ? n / a : 1), "cpus %d active %d: T %d", cpus, a, T);
                sum += T;
            }
            const int m = k < n ? k : n;
            int closed = k > n ? k - n : 0;
            for (int j = 1; j <= n; ++j)
                closed += m < n / j ? m : n / j;
            CHECK(sum == closed, "cpus %d k %d: %d threads, closed form %d", cpus, k, sum, closed);
            /* with one driver each: between 2 k threads and what k copies alone would take */
            CHECK(sum + k >= 2 * k && sum + k <= k * (n + 1), "cpus %d k %d: %d threads with the drivers", cpus, k, sum + k);
            if (n == 8 && k == 8)
                CHECK(sum + k == 28, "cpus %d: eight copies together hold %d threads", cpus, sum + k);
            CHECK(k == 1 ? sum == n : sum > n, "cpus %d k %d: %d threads against n = %d", cpus, k, sum, n);
            if (n == 8)
                CHECK(sum == sums8[k - 1], "cpus %d k %d: %d threads, table %d", cpus, k, sum, sums8[k - 1]);
        }
    }
    CHECK(mm_hostcopy_threads(16, 0) == 8 && mm_hostcopy_threads(0, 1) == 1 && mm_hostcopy_threads(16, -3) == 8, "degenerate arguments");
    return cases;
}

/* ---- protocol ---- */

struct FakeTransport {
    const unsigned char *src;
    size_t chunk;
    unsigned char *slots[kHostcopyRing];
    struct Pending {
        size_t off = 0, len = 0;
        int not_ready = 0;
        bool filled = true;
    } pending[kHostcopyRing];
    uint32_t rng;
    long issue_calls = 0, done_answers = 0;
    long fail_issue_at = -1, fail_query_at = -1; /* chunk index */

    FakeTransport(const unsigned char *s, size_t c, uint32_t seed) : src(s), chunk(c), rng(seed * 2u + 1u)
    {
        for (auto &p : slots) {
            p = (unsigned char *)std::malloc(chunk);
            if (!p)
                std::abort();
        }
    }
    ~FakeTransport()
    {
        for (auto &p : slots)
            std::free(p);
    }
    FakeTransport(const FakeTransport &) = delete;
    FakeTransport &operator=(const FakeTransport &) = delete;

    const void *slot(int s) const { return slots[s]; }
    int issue(int s, size_t off, size_t len)
    {
        const long i = issue_calls++;
        CHECK(s == (int)(i % kHostcopyRing) && off == (size_t)i * chunk && len >= 1 && len <= chunk, "issue %ld: slot %d off %zu len %zu",
              i, s, off, len);
        CHECK(pending[s].filled, "issue %ld: slot %d issued again before its last fill was seen", i, s);
        if (i == fail_issue_at)
            return 701;
        rng = rng * 1664525u + 1013904223u;
        pending[s].off = off;
        pending[s].len = len;
        pending[s].not_ready = (int)(rng >> 29);
        pending[s].filled = false;
        return 0;
    }
    int query(int s)
    {
        Pending &p = pending[s];
        CHECK(!p.filled && s == (int)(done_answers % kHostcopyRing), "query of slot %d with nothing in flight", s);
        if (p.filled)
            return 703;
        if (p.not_ready > 0) {
            --p.not_ready;
            return kHostcopyNotReady;
        }
        if (done_answers == fail_query_at)
            return 702;
        std::memcpy(slots[s], src + p.off, p.len); /* the "DMA" lands now */
        p.filled = true;
        ++done_answers;
        return 0;
    }
};

struct Arena {
    size_t bytes, shift;
    unsigned char *buf;
    static constexpr size_t kPad = 256;
    Arena(size_t b, size_t s) : bytes(b), shift(s), buf((unsigned char *)std::malloc(b + 2 * kPad))
    {
        if (!buf)
            std::abort();
        std::memset(buf, 0x5a, bytes + 2 * kPad);
    }
    ~Arena() { std::free(buf); }
    Arena(const Arena &) = delete;
    Arena &operator=(const Arena &) = delete;
    unsigned char *dst() const { return buf + 64 + shift; }
    /* [0, from) of the destination holds the source (maybe: or, byte by byte, was never written), everything else in the buffer
     * is still 0x5a */
    bool intact(const unsigned char *src, size_t from, bool maybe = false) const
    {
        const size_t d0 = 64 + shift;
        for (size_t i = 0; i < d0; ++i)
            if (buf[i] != 0x5a)
                return false;
        for (size_t i = 0; i < from; ++i)
            if (buf[d0 + i] != src[i] && !(maybe && buf[d0 + i] == 0x5a))
                return false;
        for (size_t i = d0 + from; i < bytes + 2 * kPad; ++i)
            if (buf[i] != 0x5a)
                return false;
        return true;
    }
};

static unsigned char *make_source(size_t bytes)
{
    unsigned char *src = (unsigned char *)std::malloc(bytes);
    if (!src)
        std::abort();
    for (size_t i = 0; i < bytes; ++i)
        src[i] = pattern(i);
    return src;
}

static void protocol_case(const unsigned char *src, size_t bytes, size_t chunk, int T, size_t shift, uint32_t seed)
{
    Arena ar(bytes, shift);
    FakeTransport tr(src, chunk, seed);
    const mm_hostcopy_result r = mm_hostcopy_ring(tr, ar.dst(), bytes, chunk, T);
    const long nc = (long)mm_hostcopy_chunks(bytes, chunk);
    CHECK(r.started && r.error == 0, "bytes %zu chunk %zu T %d shift %zu: started %d error %d", bytes, chunk, T, shift, (int)r.started, r.error);
    CHECK(tr.issue_calls == nc && tr.done_answers == nc, "bytes %zu T %d: %ld issues %ld fills of %ld", bytes, T, tr.issue_calls,
          tr.done_answers, nc);
    CHECK(ar.intact(src, bytes), "bytes %zu chunk %zu T %d shift %zu: the destination or its surroundings differ", bytes, chunk, T, shift);
}

static long protocol_small(const unsigned char *src)
{
    const size_t C = 64u << 10;
    const size_t counts[] = {1, 4095, 4096, 4097, C - 1, C, C + 1, 4 * C - 1, 4 * C, 4 * C + 1, 5 * C, 8 * C + 4097, 9 * C + 8191};
    long n = 0;
    for (size_t bytes : counts)
        for (int T : {1, 2, 3, 5, 8})
            for (size_t shift : {(size_t)0, (size_t)4, (size_t)60})
                protocol_case(src, bytes, C, T, shift, (uint32_t)++n);
    return n;
}

static long protocol_real_chunk(const unsigned char *src)
{
    long n = 0;
    for (size_t bytes : {kHostcopyChunk + 4, 4 * kHostcopyChunk + 4})
        for (int T : {3, 8})
            protocol_case(src, bytes, kHostcopyChunk, T, 4, (uint32_t)(1000 + ++n));
    return n;
}

/* ---- failures ---- */

struct ThrowingSpawn {
    int at;
    template <class F>
    std::thread operator()(F &f, int t) const
    {
        if (t == at)
            throw std::runtime_error("no more threads");
        return std::thread(f, t);
    }
};

static long failures(const unsigned char *src)
{
    const size_t C = 64u << 10, bytes = 9 * C + 8191;
    const long last = (long)mm_hostcopy_chunks(bytes, C) - 1;
    const int T = 3;
    long n = 0;
    for (int kind = 0; kind < 2; ++kind)
        for (long j : {0L, 3L, 4L, last}) {
            Arena ar(bytes, 4);
            FakeTransport tr(src, C, (uint32_t)(2000 + ++n));
            (kind == 0 ? tr.fail_issue_at : tr.fail_query_at) = j;
            const mm_hostcopy_result r = mm_hostcopy_ring(tr, ar.dst(), bytes, C, T);
            CHECK(r.started && r.error == (kind == 0 ? 701 : 702), "%s fails at chunk %ld: started %d error %d", kind == 0 ? "issue" : "query", j,
                  (int)r.started, r.error);
            /* a worker that sees the failure while it waits leaves, even if its chunk has been published since: of the published
             * chunks every byte is the source's or untouched, beyond them nothing is written */
            const long pub = tr.done_answers;
            CHECK(pub <= j && (kind == 0 || pub == j), "%s fails at chunk %ld: %ld chunks published", kind == 0 ? "issue" : "query", j, pub);
            CHECK(kind == 1 || tr.issue_calls == j + 1, "issue fails at chunk %ld: %ld issues", j, tr.issue_calls);
            CHECK(ar.intact(src, (size_t)pub * C, true), "%s fails at chunk %ld: foreign bytes in the published chunks, or bytes written beyond them",
                  kind == 0 ? "issue" : "query", j);
        }
    for (int at : {0, 4}) {
        const int T5 = 5;
        Arena ar(bytes, 4);
        FakeTransport tr(src, C, (uint32_t)(2000 + ++n));
        const mm_hostcopy_result r = mm_hostcopy_ring(tr, ar.dst(), bytes, C, T5, ThrowingSpawn{at});
        CHECK(!r.started && r.error == 0, "thread %d of %d cannot start: started %d error %d", at, T5, (int)r.started, r.error);
        CHECK(tr.issue_calls == 0 && ar.intact(src, 0), "thread %d of %d cannot start: %ld issues, or bytes written", at, T5, tr.issue_calls);
    }
    return n;
}

int main()
{
    const long slices = plan_slices(), chunks = plan_chunks(), decisions = plan_decisions();
    const long budgets = budget();
    unsigned char *src = make_source(4 * kHostcopyChunk + 4);
    const long small = protocol_small(src), real = protocol_real_chunk(src), fails = failures(src);
    std::free(src);
    std::printf("slices %ld chunk tilings %ld decisions %ld budgets %ld protocol %ld real chunk %ld failures %ld failed %ld\n", slices, chunks,
                decisions, budgets, small, real, fails, g_failed);
    return g_failed ? 1 : 0;
}
