/* AddressSanitizer / UBSan harness for the host arithmetic of include/pawsome_video.h (pdog_time_axis, pdog_fps_table):
 * the cases of tests/test_video_cpu.py with output buffers of EXACTLY the reported size on the heap, so a write past the
 * count is caught; error cases get a one-element buffer that must stay untouched.  Built and run by tools/asan_video.sh. */
#include "pawsome_dog.h"
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); ++failures; } } while (0)

static void time_axis_case(double start, double stop, double fps, int want_n)
{
    int n = -77;
    CHECK(pdog_time_axis(start, stop, fps, NULL, 0, &n) == PDOG_OK && (want_n < 0 || n == want_n));
    double *ts = (double *)malloc(sizeof(double) * (size_t)n);
    int n2 = -77;
    CHECK(pdog_time_axis(start, stop, fps, ts, n, &n2) == PDOG_OK && n2 == n);
    CHECK(ts[0] == start && (n == 1 || fabs(ts[n - 1] - stop) <= 1e-9 * fmax(1.0, fabs(stop))));
    for (int j = 1; j < n; ++j) CHECK(ts[j] > ts[j - 1]);
    if (n > 1) CHECK(pdog_time_axis(start, stop, fps, ts, n - 1, &n2) == PDOG_E_ARG && n2 == n);
    free(ts);
}

static void fps_case(double rate, int n_frames, double start, double stop, double fps, const int *head, int n_head)
{
    int n = -77;
    CHECK(pdog_fps_table(rate, n_frames, start, stop, fps, NULL, 0, &n) == PDOG_OK && n >= 1);
    int32_t *ix = (int32_t *)malloc(sizeof(int32_t) * (size_t)n);
    int n2 = -77;
    CHECK(pdog_fps_table(rate, n_frames, start, stop, fps, ix, n, &n2) == PDOG_OK && n2 == n);
    for (int j = 0; j < n; ++j) CHECK(ix[j] >= 0 && ix[j] < n_frames && (j == 0 || ix[j] >= ix[j - 1]));
    for (int j = 0; j < n_head && j < n; ++j) CHECK(ix[j] == head[j]);
    if (n > 1) CHECK(pdog_fps_table(rate, n_frames, start, stop, fps, ix, n - 1, &n2) == PDOG_E_ARG && n2 == n);
    free(ix);
}

int main(void)
{
    static const double pairs[9][2] = {{30, 24}, {30, 12}, {25, 24}, {60, 24}, {24, 30}, {30, 30}, {29.97, 24}, {50, 12.5}, {30, 7.5}};
    static const double starts[5] = {0.0, 0.2, 0.21, 0.5, 1.234};
    static const int h3024[7] = {0, 1, 3, 4, 5, 6, 8}, h3012[5] = {1, 3, 6, 8, 11}, h2430[8] = {0, 1, 1, 2, 3, 4, 5, 5};
    /* the time axis: ties to even, one stamp, a day at 24 per second */
    time_axis_case(0.0, 1.0, 2.5, 2); time_axis_case(0.0, 1.0, 3.5, 4); time_axis_case(1.0, 2.0, 4.5, 4);
    time_axis_case(7.0, 8.0, 1.0, 1); time_axis_case(0.2, 1.7, 24.0, 36); time_axis_case(0.0, PDOG_DEFAULT_STOP, 24.0, 2073600);
    time_axis_case(0.0, 10.0, 0.1, 1); time_axis_case(1.0, 2.0, 29.97, 30);
    /* the fps rule: the nine pairs, start on and between frame times, stop inside and far beyond the stack */
    for (int p = 0; p < 9; ++p)
        for (int s = 0; s < 5; ++s) {
            fps_case(pairs[p][0], 2000, starts[s], starts[s] + 3.0, pairs[p][1], NULL, 0);
            fps_case(pairs[p][0], 2000, starts[s], PDOG_DEFAULT_STOP, pairs[p][1], NULL, 0);
        }
    fps_case(30, 2000, 0.0, PDOG_DEFAULT_STOP, 24, h3024, 7);
    fps_case(30, 2000, 0.0, PDOG_DEFAULT_STOP, 12, h3012, 5);
    fps_case(24, 2000, 0.0, PDOG_DEFAULT_STOP, 30, h2430, 8);
    fps_case(30, 1, 0.0, 10.0, 24, NULL, 0); fps_case(30, 61, 2.0, 10.0, 30, NULL, 0);
    /* errors: the outputs stay untouched */
    {
        static const double bad_t[8][3] = {{1, 1, 24}, {2, 1, 24}, {0, 1, 0}, {0, 1, -3}, {0, 1, 0.5}, {0, 1, 0.25}, {0, 1e12, 1e3}, {0, NAN, 24}};
        static const double bad_f[9][5] = {{0, 100, 0, 1, 24}, {-30, 100, 0, 1, 24}, {30, 0, 0, 1, 24}, {30, -5, 0, 1, 24}, {30, 100, -0.1, 1, 24},
                                           {30, 100, 1, 1, 24}, {30, 100, 0, 1, 0}, {30, 60, 2.0, 3.0, 24}, {NAN, 100, 0, 1, 24}};
        double *ts = (double *)malloc(sizeof(double));
        int32_t *ix = (int32_t *)malloc(sizeof(int32_t));
        int n = -77;
        *ts = -77.0; *ix = -77;
        for (int k = 0; k < 8; ++k) CHECK(pdog_time_axis(bad_t[k][0], bad_t[k][1], bad_t[k][2], ts, 1, &n) == PDOG_E_ARG);
        for (int k = 0; k < 9; ++k) CHECK(pdog_fps_table(bad_f[k][0], (int)bad_f[k][1], bad_f[k][2], bad_f[k][3], bad_f[k][4], ix, 1, &n) == PDOG_E_ARG);
        CHECK(pdog_time_axis(0, 1, 24, NULL, 0, NULL) == PDOG_E_ARG && pdog_fps_table(30, 100, 0, 1, 24, NULL, 0, NULL) == PDOG_E_ARG);
        CHECK(n == -77 && *ts == -77.0 && *ix == -77 && strlen(pdog_last_error()) > 0);
        free(ts); free(ix);
    }
    printf(failures ? "video harness: %d FAILED\n" : "video harness: ok (%d failures)\n", failures);
    return failures != 0;
}
