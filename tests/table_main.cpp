// A stand-alone program over the host side of the table walks (csrc/pdog_math.cpp, no GPU): check_table_walk judges the walk
// the arguments describe, fill_table lays it out into a heap buffer of exactly the words the layout takes, and the words are
// printed for tests/test_table_cpu.py to hold against its own restatement.  The same source builds under AddressSanitizer and
// UBSan: a cell or a length written one word too far is the run's failure.
//   table_main n_frames n_rows n_steps windows first entry...      (windows = 0: the rows as given)
// prints "len <per row> max <max_len>" and "words <cells, then lengths>"; a refused walk prints "error <text>" and exits 2.
#include "pdog_math.cpp"

#include <cstdio>
#include <cstdlib>
#include <memory>

int main(int argc, char **argv)
{
    if (argc < 6) return 1;
    const int n_frames = std::atoi(argv[1]), n_rows = std::atoi(argv[2]), n_steps = std::atoi(argv[3]), windows = std::atoi(argv[4]),
              first = std::atoi(argv[5]);
    if (n_rows < 0 || n_steps < 0 || argc != 6 + n_rows * n_steps) return 1;
    std::unique_ptr<int32_t[]> table(new int32_t[(size_t)n_rows * n_steps]);
    for (int i = 0; i < n_rows * n_steps; ++i) table[i] = std::atoi(argv[6 + i]);
    std::vector<int32_t> len;
    pdog::TableWalk w{"table_main", 8, n_frames, 8, 64, table.get(), n_steps, n_rows, windows ? windows : 1, first, 0, 0};
    if (pdog::check_table_walk(w, len)) {
        std::printf("error %s\n", pdog_last_error());
        return 2;
    }
    if ((int)len.size() != n_rows) return 1;
    const pdog::TableShape s{n_steps, n_rows, w.max_len, windows};
    const size_t cells = pdog::table_cells(s), n = cells + (size_t)n_rows;
    std::unique_ptr<int32_t[]> words(new int32_t[n]);
    pdog::fill_table(table.get(), len.data(), s, words.get());
    std::printf("len");
    for (int r = 0; r < n_rows; ++r) std::printf(" %d", len[r]);
    std::printf(" max %d\nwords", w.max_len);
    for (size_t i = 0; i < n; ++i) std::printf(" %d", words[i]);
    std::printf("\n");
    return 0;
}
