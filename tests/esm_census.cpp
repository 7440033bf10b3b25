// The pieces of a pointer array as the edge softmax kernels walk them (csrc/edge_softmax.hip:
// esm_fwd_kernel, esm_bwd_kernel, esm_colsum_kernel), from csrc/token_items.h's own functions:
// this program includes that header alone (plain C++17, no HIP), finds every item's first row by
// a plain binary search, takes the head piece from cont_piece, the owned rows from row_owned and
// their pieces from row_piece, all under CutAtEnd.  test_esm_corners_cpu.py compares the output
// with the census of tests/esm_corner_graph.py, which restates the rule on the tokens.
//
//   esm_census FILE CHUNK...   FILE: a pointer array, whitespace-separated
//
// Prints one line per piece: `chunk item kind row sb se`, kind H (head: the continuation of the
// row before the item's first owned one, only when it holds an edge), W (an owned row that ends
// in the item, empty rows included) or T (an owned row cut at the item's end, also when the item
// holds none of its edges); then `items chunk n`.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <vector>

#include "token_items.h"

using namespace maxk;

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    std::ifstream in(argv[1]);
    std::vector<int32_t> ptr;
    for (long long v; in >> v;) ptr.push_back((int32_t)v);
    if (ptr.empty() || ptr[0] != 0 || !std::is_sorted(ptr.begin(), ptr.end())) return 2;
    const int n = (int)ptr.size() - 1;
    const int64_t num_e = ptr[n], total = (int64_t)n + num_e;
    for (int a = 2; a < argc; ++a) {
        const int chunk = std::atoi(argv[a]);
        if (chunk <= 0) return 2;
        const int n_items = token_items(n, num_e, chunk);
        for (int item = 0; item < n_items; ++item) {
            const int64_t d0 = (int64_t)item * chunk;
            const int64_t d1 = std::min<int64_t>(d0 + chunk, total);
            int lo = 0, hi = n;  // the first row whose token is >= d0
            while (lo < hi) {
                const int mid = lo + (hi - lo) / 2;
                if ((int64_t)ptr[mid] + mid >= d0) hi = mid; else lo = mid + 1;
            }
            const int r = lo;
            if (r > 0) {
                const RowPiece p = cont_piece(CutAtEnd{}, d0 - r, d1, r, ptr[r]);
                if (p.sb < p.se)
                    std::printf("%d %d H %d %lld %lld\n", chunk, item, r - 1, (long long)p.sb,
                                (long long)p.se);
            }
            for (int q = r; q < n && row_owned(d1, q, ptr[q]); ++q) {
                const RowPiece p = row_piece(CutAtEnd{}, d1, q, ptr[q], ptr[q + 1]);
                std::printf("%d %d %c %d %lld %lld\n", chunk, item, p.se == ptr[q + 1] ? 'W' : 'T',
                            q, (long long)p.sb, (long long)p.se);
            }
        }
        std::printf("items %d %d\n", chunk, n_items);
    }
    return 0;
}
