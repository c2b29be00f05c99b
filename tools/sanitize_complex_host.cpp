// Stand-alone check of the argument validation of the complex-batch entry points (csrc/complex_build.hip): every
// bad call must return -1 before anything is launched or dereferenced. Runs on the CPU, no GPU needed:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//       pointvs_amd/csrc/complex_build.hip pointvs_amd/csrc/common.cpp -x hip pointvs_amd/csrc/profile.cpp \
//       -x c++ tools/sanitize_complex_host.cpp -o /tmp/sanitize_complex_host && /tmp/sanitize_complex_host
#include <cstdio>
#include <cstdint>
#include <cstring>
#include "../include/pvs_egnn.h"
int main() {
    int bad = 0;
    bad += pvs_complex_batch_workspace_bytes(4, 1000) < 1000;
    bad += pvs_complex_batch_workspace_bytes(4, -5) != 256;
    PvsComplexPool pool;
    memset(&pool, 0, sizeof pool);
    int32_t dummy[16] = {0};
    // every argument check must return -1 before anything is launched or dereferenced
    bad += pvs_complex_batch_count(nullptr, dummy, nullptr, 1, 10, 4.0, 1, dummy, dummy, dummy, 4096, nullptr) != -1;
    bad += pvs_complex_batch_count(&pool, dummy, nullptr, 1, 10, 4.0, 1, dummy, dummy, dummy, 4096, nullptr) != -1;
    double xyz[3] = {0, 0, 0};
    pool.rec_xyz = pool.lig_xyz = xyz;
    pool.rec_types = pool.lig_types = pool.rec_z = pool.lig_z = pool.rec_ptr = pool.lig_ptr = dummy;
    pool.n_rec = pool.n_lig = 1;
    bad += pvs_complex_batch_count(&pool, dummy, nullptr, 0, 10, 4.0, 1, dummy, dummy, dummy, 4096, nullptr) != -1;
    bad += pvs_complex_batch_count(&pool, dummy, nullptr, 1, 10, 4.0, 1, dummy, dummy, dummy, 8, nullptr) != -1;
    bad += pvs_complex_batch_fill(&pool, dummy, nullptr, nullptr, 1, 10, 5, 1, 12, 1, nullptr, dummy, dummy, nullptr,
                                  nullptr, nullptr, nullptr, nullptr, dummy, dummy, 4096, nullptr) != -1;
    bad += pvs_complex_batch_fill(&pool, dummy, nullptr, nullptr, 1, 10, 5, 0, 0, 1, nullptr, dummy, dummy, nullptr,
                                  nullptr, nullptr, nullptr, nullptr, dummy, dummy, 4096, nullptr) != -1;
    bad += pvs_complex_edges(0, 5, 1, dummy, dummy, dummy, dummy, dummy, dummy, nullptr, dummy, nullptr, nullptr, dummy, nullptr) != -1;
    bad += pvs_complex_edges(5, 0, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != 0;
    bad += pvs_complex_edges(5, 3, 1, nullptr, dummy, dummy, dummy, dummy, dummy, nullptr, dummy, nullptr, nullptr, dummy, nullptr) != -1;
    printf("last error: %s\n%s\n", pvs_last_error(), bad ? "FAILED" : "ok");
    return bad;
}
