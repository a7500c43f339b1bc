// A stand-alone program over the run-time loader (csrc/pdog_dl.hpp, no GPU, no RCCL): it opens the first of the names it is
// given, resolves the symbols it is given, and prints what the loader kept for tests/test_group_open_cpu.py to compare.  The
// same source builds under AddressSanitizer and UBSan: a null appended to the error text is the run's failure.
//   group_open_main what n_names name... symbol...
// prints "handle <0|1>", "symbol <name> <0|1>" per symbol and "error <text>" (the text may be empty).
#include "pdog_dl.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

int main(int argc, char **argv)
{
    if (argc < 3) return 1;
    const char *what = argv[1];
    const int n_names = std::atoi(argv[2]);
    if (n_names < 0 || argc < 3 + n_names) return 1;
    const std::vector<const char *> names(argv + 3, argv + 3 + n_names);
    pdog::DlLibrary lib;
    lib.open_first(what, names);
    std::printf("handle %d\n", lib.handle ? 1 : 0);
    if (lib.handle)
        for (int i = 3 + n_names; i < argc; ++i) std::printf("symbol %s %d\n", argv[i], lib.symbol(what, argv[i]) ? 1 : 0);
    std::printf("error %s\n", lib.error.c_str());
    return 0;
}
