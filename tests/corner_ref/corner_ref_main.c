/* Stand-alone driver of the CPU reference (tests/corner_ref/corner_ref.c) for a sanitizer build: reads one
 * problem from a file, detects, and prints the status, the count and every output word in hex, one corner
 * per line.
 * File: int32 rows, cols, method, f, strongest, list_cap, capacity, has_roi, roi[4]; float min_quality;
 * img [rows][cols] u8. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

int corner_ref_detect(const uint8_t* img, int rows, int cols, int method, int f, float min_quality, int strongest, const int* roi,
                      int list_cap, float* metric_plane, float* loc, float* metric, int capacity, int* n_out);

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: corner_ref_main problem.bin\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t h[12];
    float min_quality;
    if (fread(h, 4, 12, f) != 12 || fread(&min_quality, 4, 1, f) != 1) return 2;
    const int rows = h[0], cols = h[1], method = h[2], fs = h[3], strongest = h[4], list_cap = h[5], capacity = h[6], has_roi = h[7];
    if (rows < 1 || cols < 1 || rows > 4096 || cols > 4096 || fs < 3 || fs > 15 || !(fs & 1) || capacity < 0 || capacity > 1000000) return 2;
    const size_t px = (size_t)rows * cols;
    uint8_t* img = malloc(px);
    float* loc = malloc(sizeof(float) * 2 * ((size_t)capacity + 1));
    float* met = malloc(sizeof(float) * ((size_t)capacity + 1));
    if (!img || !loc || !met || fread(img, 1, px, f) != px) return 2;
    fclose(f);
    int roi[4] = {h[8], h[9], h[10], h[11]}, n = 0;
    const int rc = corner_ref_detect(img, rows, cols, method, fs, min_quality, strongest, has_roi ? roi : 0, list_cap, 0, loc, met, capacity, &n);
    if (rc < 0) return 2;
    printf("%d %d\n", rc, n);
    for (int i = 0; rc == 0 && i < n; ++i) printf("%08x %08x %08x\n", bits(loc[2 * i]), bits(loc[2 * i + 1]), bits(met[i]));
    free(img); free(loc); free(met);
    return 0;
}
