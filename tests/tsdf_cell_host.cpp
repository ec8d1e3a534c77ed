// Host driver of pyslam_amd/csrc/hv_tsdf_cell.h for tests/test_tsdf_cell_cpu.py: the header's arithmetic part compiled without HIP.
//   tsdf_cell_host <in> <out>
// in:  int64 n, then n records {double p[3], voxel_length, f[8]; float rf[3], ff[8], pad}
// out: n records {int32 g0[3], ok; double r[3], phi, phi_grad, e[3]; float lerp_f, pad}, then the corner table int32 [8][3]
// The trilinear forms take the r the locate produced (zeros where it refused the point).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "hv_tsdf_cell.h"

struct In {
    double p[3], voxel_length, f[8];
    float rf[3], ff[8], pad;
};
struct Out {
    int32_t g0[3], ok;
    double r[3], phi, phi_grad, e[3];
    float lerp_f, pad;
};
static_assert(sizeof(In) == 144 && sizeof(Out) == 88, "the records the test's numpy dtypes describe");

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *fi = fopen(argv[1], "rb");
    if (fi == nullptr) return 3;
    int64_t n = 0;
    if (fread(&n, sizeof(n), 1, fi) != 1 || n < 0 || n > (1 << 24)) return 4;
    std::vector<In> in((size_t)n);
    if (fread(in.data(), sizeof(In), (size_t)n, fi) != (size_t)n) return 5;
    fclose(fi);
    std::vector<Out> out((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        const In &a = in[(size_t)i];
        Out &o = out[(size_t)i];
        o.ok = hv_cell_locate(a.p, a.voxel_length, o.g0, o.r) ? 1 : 0;
        double r[3];
        for (int k = 0; k < 3; ++k) r[k] = o.ok ? o.r[k] : 0.0;
        o.phi = hv_cell_lerp(r, a.f);
        hv_cell_lerp_grad(r, a.f, o.phi_grad, o.e);
        o.lerp_f = hv_cell_lerp(a.rf, a.ff);
        o.pad = 0.0f;
    }
    int32_t corners[8][3];
    for (int c = 0; c < 8; ++c) {
        int sx, sy, sz;
        hv_cell_corner(c, sx, sy, sz);
        corners[c][0] = sx, corners[c][1] = sy, corners[c][2] = sz;
    }
    FILE *fo = fopen(argv[2], "wb");
    if (fo == nullptr) return 7;
    if (fwrite(out.data(), sizeof(Out), (size_t)n, fo) != (size_t)n || fwrite(corners, sizeof(corners), 1, fo) != 1) return 8;
    fclose(fo);
    return 0;
}
