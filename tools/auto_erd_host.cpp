// Stand-alone host program around auto_erd_pixel (csrc/auto_erd_pixel.h), the per-pixel body of auto_erd_kernel: the same text
// compiled by the host compiler, so that its walk can be run under -fsanitize=address,undefined and compared with
// oracle/erd_oracle.py without a device (tests/test_metrics_edges_cpu.py builds and runs it).
//
//   auto_erd_host SAMPLES
//
// SAMPLES is a text file with one pixel per line: `rule erd_positive n v_0 ... v_{n-1}`; the values are anything strtod reads
// (hexadecimal floats, "nan", "inf", "-inf").  One line of n characters '0' / '1' (the accept mask) is printed per pixel.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "auto_erd_pixel.h"

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: %s SAMPLES\n", argv[0]);
        return 2;
    }
    std::FILE* in = std::fopen(argv[1], "r");
    if (!in) {
        std::perror(argv[1]);
        return 2;
    }
    int rule, positive, n;
    long pixels = 0;
    while (std::fscanf(in, "%d %d %d", &rule, &positive, &n) == 3) {
        if (n < 2 || n > inr::ERD_MAXN || (rule != 1 && rule != 2)) {
            std::fprintf(stderr, "pixel %ld: bad header (rule %d, n %d)\n", pixels, rule, n);
            return 2;
        }
        // exactly n values on the heap, so that a read or write past them is seen by the address sanitizer
        std::vector<double> values(n);
        std::vector<float> accept(n);
        char token[64];
        for (int i = 0; i < n; ++i) {
            if (std::fscanf(in, "%63s", token) != 1) {
                std::fprintf(stderr, "pixel %ld: %d values expected\n", pixels, n);
                return 2;
            }
            values[i] = std::strtod(token, nullptr);
        }
        const double majority = (2.0 / 3.0) * (double)n;   // as launch_auto_erd
        inr::auto_erd_pixel(accept.data(), values.data(), n, rule, majority, positive != 0);
        for (int i = 0; i < n; ++i) std::putchar(accept[i] == 1.f ? '1' : (accept[i] == 0.f ? '0' : '?'));
        std::putchar('\n');
        ++pixels;
    }
    std::fclose(in);
    return 0;
}
