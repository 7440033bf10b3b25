// The cut rules of csrc/token_items.h, checked on the CPU: this program includes that header
// alone (plain C++17, no HIP), walks every item of a set of pointer arrays the way the kernels
// do -- a plain binary search for the item's first row, then under CutAtEnd the header's item
// driver walk_cut_item, the function the kernels run, and under CutHubRows its cont_piece /
// row_piece -- and compares who walks which edge with the rules' definition on the tokens.
//
//   partition_check [FILE...]   each FILE: one more pointer array, whitespace-separated
//
// Exit status 0 when every check holds; the first failure is printed and exits 1.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <type_traits>
#include <vector>

#include "token_items.h"

using namespace maxk;
using Ptr = std::vector<int32_t>;

#define CHECK(cond, ...)                                          \
    do {                                                          \
        if (!(cond)) {                                            \
            std::printf("FAILED %s:%d  %s\n  ", __FILE__, __LINE__, #cond); \
            std::printf(__VA_ARGS__);                             \
            std::printf("\n");                                    \
            std::exit(1);                                         \
        }                                                         \
    } while (0)

static Ptr from_degrees(const std::vector<int> &deg) {
    Ptr p(deg.size() + 1, 0);
    for (size_t i = 0; i < deg.size(); ++i) p[i + 1] = p[i] + deg[i];
    return p;
}

// the first r in [0, n] whose token r + ptr[r] is >= d (wave_first_row_token's contract)
static int first_row_token(const Ptr &ptr, int n, int64_t d) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if ((int64_t)ptr[mid] + mid >= d) hi = mid; else lo = mid + 1;
    }
    return lo;
}

struct Walk {
    std::vector<int> walker;    // per edge: the item that walked it (-1: none)
    std::vector<int> owner;     // per row: the item that owned it (-1: none)
    std::vector<int> slab_row;  // per item: the row it continues (-1: none)
    std::vector<int64_t> tokens;  // per item: rows owned + edges walked
};

template <class Rule>
static Walk walk(const Ptr &ptr, int chunk, const char *what) {
    const int n = (int)ptr.size() - 1;
    const int64_t num_e = ptr[n];
    const int n_items = token_items(n, num_e, chunk);
    constexpr bool HUBS = std::is_same<Rule, CutHubRows>::value;
    Walk w{std::vector<int>((size_t)num_e, -1), std::vector<int>((size_t)n, -1),
           std::vector<int>((size_t)n_items, -1), std::vector<int64_t>((size_t)n_items, 0)};
    auto mark = [&](int item, const RowPiece &p, int q) {
        CHECK(p.sb >= ptr[q] && p.se <= ptr[q + 1], "%s chunk %d item %d row %d: piece [%lld, %lld) "
              "leaves the row", what, chunk, item, q, (long long)p.sb, (long long)p.se);
        for (int64_t e = p.sb; e < p.se; ++e) {
            CHECK(w.walker[(size_t)e] < 0, "%s chunk %d: edge %lld walked by items %d and %d", what,
                  chunk, (long long)e, w.walker[(size_t)e], item);
            w.walker[(size_t)e] = item;
        }
        if (p.se > p.sb) w.tokens[(size_t)item] += p.se - p.sb;
    };
    const int64_t total = (int64_t)n + num_e;
    for (int item = 0; item < n_items; ++item) {
        // ItemRange, as item_range() builds it on the device
        const int64_t d0 = (int64_t)item * chunk;
        const int64_t d1 = std::min<int64_t>(d0 + chunk, total);
        const int r = first_row_token(ptr, n, d0);
        const ItemRange it{d0, d1, r, d0 - r};
        auto own = [&](int q) {
            CHECK(w.owner[(size_t)q] < 0, "%s chunk %d: row %d owned twice", what, chunk, q);
            w.owner[(size_t)q] = item;
            w.tokens[(size_t)item] += 1;
        };
        if constexpr (!HUBS) {  // the driver the kernels run
            walk_cut_item(ptr.data(), n, it,
                          [&](int q, int64_t sb, int64_t se, int64_t re, bool cont) {
                const RowPiece p{sb, se, false};
                CHECK(q >= 0 && q < n && cont == (q == r - 1) && re == ptr[q + 1],
                      "%s chunk %d item %d: the driver reports row %d", what, chunk, item, q);
                const RowPiece a = any_piece(CutAtEnd{}, d0, d1, q, ptr[q], ptr[q + 1]);
                if (cont) {
                    if (p.sb < p.se) {
                        mark(item, p, q);
                        w.slab_row[(size_t)item] = q;
                    }
                    CHECK((a.sb >= a.se && p.sb >= p.se) || (a.sb == p.sb && a.se == p.se),
                          "%s chunk %d item %d: any_piece differs from cont_piece", what, chunk,
                          item);
                } else {
                    own(q);
                    CHECK(a.sb == p.sb && a.se == p.se, "%s chunk %d row %d: any_piece differs "
                          "from row_piece", what, chunk, q);
                    mark(item, p, q);
                }
            });
            continue;
        }
        if (r > 0) {
            const RowPiece p = cont_piece(CutHubRows{}, it.p_lo, d1, r, ptr[r - 1], ptr[r], chunk);
            if (p.hub && p.sb < p.se) {
                mark(item, p, r - 1);
                w.slab_row[(size_t)item] = r - 1;
            }
        }
        for (int q = r; q < n; ++q) {
            if (!row_owned(d1, q, ptr[q])) break;
            own(q);
            const RowPiece p = row_piece(CutHubRows{}, d1, q, ptr[q], ptr[q + 1], chunk);
            CHECK(p.hub == (ptr[q + 1] - ptr[q] > chunk), "%s chunk %d row %d: hub flag", what,
                  chunk, q);
            mark(item, p, q);
        }
    }
    return w;
}

// The rules' definition on the tokens: row q's token is q + ptr[q], its edge e's e + q + 1,
// token t belongs to item t / chunk.
template <class Rule>
static void check(const Ptr &ptr, int chunk, const char *what) {
    constexpr bool HUBS = std::is_same<Rule, CutHubRows>::value;
    const int n = (int)ptr.size() - 1;
    const Walk w = walk<Rule>(ptr, chunk, what);
    const int n_items = (int)w.slab_row.size();
    std::vector<int> expect_cont((size_t)n_items, -1);
    for (int q = 0; q < n; ++q) {
        const int own = (int)(((int64_t)q + ptr[q]) / chunk);
        CHECK(w.owner[(size_t)q] == own, "%s chunk %d: row %d owned by item %d, its token lies in "
              "item %d", what, chunk, q, w.owner[(size_t)q], own);
        const bool whole = HUBS && ptr[q + 1] - ptr[q] <= chunk;
        for (int64_t e = ptr[q]; e < ptr[q + 1]; ++e) {
            const int want = whole ? own : (int)((e + q + 1) / chunk);
            CHECK(w.walker[(size_t)e] == want, "%s chunk %d: edge %lld of row %d walked by item %d, "
                  "expected %d", what, chunk, (long long)e, q, w.walker[(size_t)e], want);
            if (want != own) {
                CHECK(expect_cont[(size_t)want] < 0 || expect_cont[(size_t)want] == q,
                      "%s chunk %d: item %d continues two rows", what, chunk, want);
                expect_cont[(size_t)want] = q;
            }
        }
    }
    // the fixup adds, per row, the slabs of the run of consecutive items whose slab_row names
    // it onto the owner's partial: those must be exactly the items that walked a piece of a row
    // they do not own, and each run must start right after the row's owner
    for (int i = 0; i < n_items; ++i) {
        CHECK(w.slab_row[(size_t)i] == expect_cont[(size_t)i], "%s chunk %d: item %d reports the "
              "continuation of row %d, its tokens say %d", what, chunk, i, w.slab_row[(size_t)i],
              expect_cont[(size_t)i]);
        const int q = w.slab_row[(size_t)i];
        if (q >= 0)
            CHECK(i > 0 && (w.slab_row[(size_t)i - 1] == q || w.owner[(size_t)q] == i - 1),
                  "%s chunk %d: item %d's slab of row %d does not follow the row's owner or "
                  "another slab of it", what, chunk, i, q);
        if (HUBS)
            CHECK(w.tokens[(size_t)i] <= 2 * (int64_t)chunk, "%s chunk %d: item %d walks %lld "
                  "tokens", what, chunk, i, (long long)w.tokens[(size_t)i]);
        else
            CHECK(w.tokens[(size_t)i] <= chunk, "%s chunk %d: item %d walks %lld tokens", what,
                  chunk, i, (long long)w.tokens[(size_t)i]);
    }
}

int main(int argc, char **argv) {
    std::vector<std::pair<std::string, Ptr>> fixed;
    fixed.push_back({"no rows", Ptr{0}});
    fixed.push_back({"one empty row", from_degrees({0})});
    fixed.push_back({"empty rows first, last and in runs",
                     from_degrees({0, 0, 0, 5, 1, 0, 0, 0, 0, 7, 0, 2, 2, 0, 0, 0, 130, 0, 3, 0, 0})});
    for (int a = 1; a < argc; ++a) {
        std::ifstream in(argv[a]);
        Ptr p;
        for (long long v; in >> v;) p.push_back((int32_t)v);
        CHECK(!p.empty() && p[0] == 0 && std::is_sorted(p.begin(), p.end()), "%s: not a pointer "
              "array", argv[a]);
        fixed.push_back({argv[a], p});
    }
    long runs = 0;
    auto both = [&](const Ptr &p, int chunk, const std::string &what) {
        check<CutAtEnd>(p, chunk, (what + " / CutAtEnd").c_str());
        check<CutHubRows>(p, chunk, (what + " / CutHubRows").c_str());
        runs += 2;
    };
    auto chunks_of = [](const Ptr &p) {
        const int len = std::max<int>(1, (int)p.size() - 1 + p.back());  // its tokens
        return std::vector<int>{1, 2, 3, 64, len, len + 1};
    };
    for (const auto &f : fixed)
        for (int chunk : chunks_of(f.second)) both(f.second, chunk, f.first);
    // the arrays stated in terms of an item size c: each runs at c and at the chunks above
    for (int c : {1, 2, 3, 64, 200}) {
        std::vector<std::pair<std::string, Ptr>> sized;
        for (int d : {c - 1, c, c + 1})
            sized.push_back({"one row of " + std::to_string(d) + " edges", from_degrees({d})});
        // a hub spanning four items, short rows around it
        sized.push_back({"a hub over four items", from_degrees({1, 0, 3 * c + c / 2 + 1, 2, 0})});
        // a hub whose last edge has an item's last token: row 0's token, the hub's (row 1) and
        // its 2 * c - 2 edges fill the first two items exactly when row 0 is empty
        if (c > 1)
            sized.push_back({"a hub ending on an item boundary", from_degrees({0, 2 * c - 2, 1, 0, 4})});
        sized.push_back({"rows near the item size", from_degrees({c, 0, c + 1, c - 1, 0, 0, c})});
        for (const auto &f : sized) {
            std::vector<int> chunks = chunks_of(f.second);
            chunks.push_back(c);
            for (int chunk : chunks) both(f.second, chunk, f.first + " (c = " + std::to_string(c) + ")");
        }
    }
    std::printf("partition_check: %ld walks ok\n", runs);
    return 0;
}
