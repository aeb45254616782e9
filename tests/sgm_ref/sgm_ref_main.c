/* Stand-alone driver of the CPU reference (tests/sgm_ref/sgm_ref.c) for a sanitizer build: reads one problem
 * from a file, runs the disparity and the reconstruction, and prints the FNV-1a hash of S's bytes, the
 * counters and the hash of the disparity map's bytes.
 * File: int32 rows, cols, dmin, D, P1, P2, U; left [rows][cols] u8; right [rows][cols] u8. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

int sgm_ref_n_counters(void);
int sgm_ref_disparity(const uint8_t* left, const uint8_t* right, int rows, int cols, int dmin, int D, int P1, int P2, int U,
                      uint16_t* S_out, float* disp, int64_t* counters);
void sgm_ref_reconstruct(const float* disp, int rows, int cols, int col_major, const double* Q, float* xyz);

static uint64_t fnv1a(const void* p, size_t n)
{
    const uint8_t* b = p;
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 0x100000001b3ull;
    return h;
}

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: sgm_ref_main problem.bin\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t h[7];
    if (fread(h, 4, 7, f) != 7) return 2;
    const int rows = h[0], cols = h[1], dmin = h[2], D = h[3], P1 = h[4], P2 = h[5], U = h[6];
    if (rows < 1 || cols < 1 || rows > 4096 || cols > 4096 || D < 8 || D > 128 || D % 8 || dmin < -1024 || dmin + D > 1024 || P1 < 0 ||
        P2 < P1 || P2 > 255 || U < 0 || U > 100)
        return 2;
    const size_t px = (size_t)rows * cols;
    const int nc = sgm_ref_n_counters();
    uint8_t* left = malloc(px);
    uint8_t* right = malloc(px);
    uint16_t* S = malloc(sizeof(uint16_t) * px * D);
    float* disp = malloc(sizeof(float) * px);
    float* xyz = malloc(sizeof(float) * 3 * px);
    int64_t* n = calloc((size_t)nc, sizeof(int64_t));
    if (!left || !right || !S || !disp || !xyz || !n || fread(left, 1, px, f) != px || fread(right, 1, px, f) != px) return 2;
    fclose(f);
    if (sgm_ref_disparity(left, right, rows, cols, dmin, D, P1, P2, U, S, disp, n)) return 2;
    const double Q[16] = {1, 0, 0, -0.5 * cols, 0, 1, 0, -0.5 * rows, 0, 0, 0, 100.0, 0, 0, 2.0, 0};
    sgm_ref_reconstruct(disp, rows, cols, 0, Q, xyz);
    sgm_ref_reconstruct(disp, cols, rows, 1, Q, xyz);        /* the same bytes read as a column-major cols x rows map */
    printf("S %016llx\nn", (unsigned long long)fnv1a(S, sizeof(uint16_t) * px * D));
    for (int i = 0; i < nc; ++i) printf(" %lld", (long long)n[i]);
    printf("\ndisp %016llx\n", (unsigned long long)fnv1a(disp, sizeof(float) * px));
    free(left); free(right); free(S); free(disp); free(xyz); free(n);
    return 0;
}
