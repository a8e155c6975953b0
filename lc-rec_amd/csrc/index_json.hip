// Host-side text formatting of `.index.json` (include/lcrec.h: lcrec_index_json_*).
//
// The reference builds one Python string per token and one list per item, then json.dump's a dict of
// N lists (index/generate_indices.py:83-92,138-145): minutes of interpreter time at 10 M items.
// Here a chunk of the int64 [n][L] index matrix becomes its JSON text in one pass over memory.
#include "common.h"

#include <thread>
#include <vector>

namespace lcrec {

// decimal digits of a signed 64-bit value, written forwards; returns the advanced pointer
static inline char *put_i64(char *p, int64_t v)
{
    uint64_t u = (uint64_t)v;
    if (v < 0) {
        *p++ = '-';
        u = 0 - u;
    }
    char tmp[20];
    int d = 0;
    do {
        tmp[d++] = (char)('0' + u % 10);
        u /= 10;
    } while (u);
    while (d) *p++ = tmp[--d];
    return p;
}

// "<id>": ["<a_i>", "<b_j>", ...]   -- at most 24 + L * 28 bytes
static inline char *put_item(char *p, int64_t item, const int64_t *row, int L)
{
    *p++ = '"';
    p = put_i64(p, item);
    *p++ = '"'; *p++ = ':'; *p++ = ' '; *p++ = '[';
    for (int l = 0; l < L; ++l) {
        if (l) { *p++ = ','; *p++ = ' '; }
        *p++ = '"'; *p++ = '<'; *p++ = (char)('a' + l); *p++ = '_';
        p = put_i64(p, row[l]);
        *p++ = '>'; *p++ = '"';
    }
    *p++ = ']';
    return p;
}

constexpr int64_t ITEM_HEAD = 26;   // quote + 20 digits (incl. sign) + quote, colon, space, bracket ... + "]"
constexpr int64_t TOKEN_MAX = 28;   // `, "<x_` (7) + 20 digits + `>"` (2), rounded

int64_t index_json_bound(int64_t n, int L) { return n * (ITEM_HEAD + (int64_t)L * TOKEN_MAX + 2) + 2; }

int64_t index_json_format(const int64_t *idx, int64_t n, int L, int64_t first_item, char *out, int64_t cap)
{
    if (n == 0) return 0;
    if (!idx || !out) return fail(LCREC_EINVAL, "index_json_format: NULL pointer");
    if (n < 0 || L < 1 || L > 26) return fail(LCREC_EINVAL, "index_json_format: need n >= 0 and 1 <= L <= 26 (got L=%d)", L);
    // Fast path: the caller's buffer covers the worst case, so the rows can be cut into independent
    // slices, each formatted by its own thread into its own worst-case window, then compacted.
    const int64_t per_item = ITEM_HEAD + (int64_t)L * TOKEN_MAX + 2;
    if (cap >= n * per_item) {
        unsigned hw = std::thread::hardware_concurrency();
        int nt = (int)(hw ? (hw > 16 ? 16 : hw) : 1);
        if (n < 65536) nt = 1;
        std::vector<int64_t> len(nt, 0);
        auto work = [&](int t) {
            const int64_t lo = n * t / nt, hi = n * (t + 1) / nt;
            char *p = out + lo * per_item;
            for (int64_t i = lo; i < hi; ++i) {
                if (i > lo) { *p++ = ','; *p++ = ' '; }
                p = put_item(p, first_item + i, idx + i * L, L);
            }
            len[t] = p - (out + lo * per_item);
        };
        if (nt == 1) {
            work(0);
            return len[0];
        }
        std::vector<std::thread> th;
        for (int t = 0; t < nt; ++t) th.emplace_back(work, t);
        for (auto &x : th) x.join();
        char *w = out;
        for (int t = 0; t < nt; ++t) {
            const int64_t lo = n * t / nt;
            if (len[t] == 0) continue;
            if (w != out) { *w++ = ','; *w++ = ' '; }
            memmove(w, out + lo * per_item, (size_t)len[t]);   // destinations never overtake sources
            w += len[t];
        }
        return w - out;
    }
    // Tight buffer: single pass with a bound check per item.
    char *p = out, *end = out + cap;
    for (int64_t i = 0; i < n; ++i) {
        if (end - p < per_item) return fail(LCREC_EWORKSPACE, "index_json_format: buffer of %lld bytes is too small", (long long)cap);
        if (i) { *p++ = ','; *p++ = ' '; }
        p = put_item(p, first_item + i, idx + i * L, L);
    }
    return p - out;
}

// ---- the reader: the strict inverse of index_json_format inside "{" ... "}" (include/lcrec.h: lcrec_index_json_parse)
namespace {

struct Scan {
    const char *p, *end, *begin;
    int64_t at() const { return p - begin; }
    bool lit(const char *s, int n)   // the next n bytes are s: consumed; otherwise nothing is
    {
        if (end - p < n || memcmp(p, s, (size_t)n) != 0) return false;
        p += n;
        return true;
    }
    // decimal digits as json.dump writes an int >= 0: no sign, no leading zero, at most INT64_MAX.  0 ok, 1 malformed, 2 overflow
    int number(int64_t *v)
    {
        if (p == end || *p < '0' || *p > '9') return 1;
        if (*p == '0' && end - p > 1 && p[1] >= '0' && p[1] <= '9') return 1;
        uint64_t u = 0;
        while (p != end && *p >= '0' && *p <= '9') {
            const unsigned d = (unsigned)(*p - '0');
            if (u > (uint64_t)INT64_MAX / 10 || (u == (uint64_t)INT64_MAX / 10 && d > (uint64_t)INT64_MAX % 10)) return 2;
            u = u * 10 + d;
            ++p;
        }
        *v = (int64_t)u;
        return 0;
    }
};

}  // namespace

int64_t index_json_parse(const char *text, int64_t len, int L, int64_t *idx_out, int64_t cap_items)
{
    if (L < 1 || L > 26) return fail(LCREC_EINVAL, "index_json_parse: need 1 <= L <= 26 (got L=%d)", L);
    if (len < 0 || cap_items < 0) return fail(LCREC_EINVAL, "index_json_parse: len=%lld, cap_items=%lld", (long long)len, (long long)cap_items);
    if (!text || (cap_items > 0 && !idx_out)) return fail(LCREC_EINVAL, "index_json_parse: NULL pointer");
    Scan s{text, text + len, text};
#define LCREC_PARSE_FAIL(what) \
    return fail(LCREC_EINVAL, "index_json_parse: byte %lld (item %lld): expected %s", (long long)s.at(), (long long)item, what)
    int64_t item = 0;
    if (!s.lit("{", 1)) LCREC_PARSE_FAIL("'{'");
    if (s.lit("}", 1)) {
        if (s.p != s.end) LCREC_PARSE_FAIL("the end of the text after '}'");
        return 0;
    }
    for (;;) {
        int64_t v;
        if (!s.lit("\"", 1)) LCREC_PARSE_FAIL("'\"' opening a key");
        const char *key = s.p;
        const int kr = s.number(&v);
        if (kr != 0 || v != item) {
            s.p = key;
            LCREC_PARSE_FAIL("the key of this item: keys are \"0\", \"1\", ... in order");
        }
        if (!s.lit("\": [", 4)) LCREC_PARSE_FAIL("'\": ['");
        if (item >= cap_items)
            return fail(LCREC_EWORKSPACE, "index_json_parse: byte %lld: item %lld does not fit in cap_items=%lld rows", (long long)s.at(),
                        (long long)item, (long long)cap_items);
        int64_t *row = idx_out + item * L;
        for (int l = 0; l < L; ++l) {
            if (l && !s.lit(", ", 2)) LCREC_PARSE_FAIL("', ' and another token: every item has L tokens");
            const char head[4] = {'"', '<', (char)('a' + l), '_'};
            if (!s.lit(head, 4)) LCREC_PARSE_FAIL("a token '\"<x_' with the prefix letter of its level");
            const int cr = s.number(&v);
            if (cr == 2) LCREC_PARSE_FAIL("a code that fits a signed 64-bit value");
            if (cr != 0) LCREC_PARSE_FAIL("a non-negative decimal code without leading zeros");
            if (!s.lit(">\"", 2)) LCREC_PARSE_FAIL("'>\"' closing a token");
            row[l] = v;
        }
        if (!s.lit("]", 1)) LCREC_PARSE_FAIL("']' after L tokens");
        ++item;
        if (s.lit(", ", 2)) continue;
        if (!s.lit("}", 1)) LCREC_PARSE_FAIL("', ' or '}'");
        if (s.p != s.end) LCREC_PARSE_FAIL("the end of the text after '}'");
        return item;
    }
#undef LCREC_PARSE_FAIL
}

}  // namespace lcrec
