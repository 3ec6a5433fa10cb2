// kd_instance_check.cpp — prints every decision of pick_kd_instance / pick_kd_batch_instance / pick_kd_walk_instance over
// the cross product of the scene traits and the calls, in the line format and order of
// tests/golden/kd_instance_choice.txt, and then the library's instance list (`table ...`).  Exit status 1 if
// kd_instance_index does not find a table row where it stands, or finds an instance the table does not hold.
// Host only; tests/test_kd_instance.py builds, runs and compares it.
#include <cstdio>

#include "../../nn_bvh_amd/csrc/kd_instance.h"

using namespace nnbvh;

static void print_instance(const KdInstance &i) {
    std::printf("<%d,%d,%d,%d,%d>", i.mode, i.patch, i.o32, i.attr, i.hostc);
}

int main() {
    for (int call = 0; call < 10; ++call)
    for (int bits = 0; bits < 256; ++bits) {
        const KdTraits t{bits >> 7 & 1, bits >> 6 & 1, bits >> 5 & 1, bits >> 4 & 1,
                         bits >> 3 & 1, bits >> 2 & 1, bits >> 1 & 1, bits & 1};
        char traits[16];
        std::snprintf(traits, sizeof traits, "%d%d%d%d%d%d%d%d", t.has_patches, t.has_extras, t.has_alpha_tex,
                      t.has_alpha_table, t.has_host_prims, t.fits32, t.offsets32, t.read_soa);
        if (call < 2) {  // single MODE
            std::printf("single %d %s ", call, traits);
            print_instance(pick_kd_instance(t, call));
            std::printf("\n");
        } else if (call < 6) {  // batch: every batch is SOA, some batch has candidates
            const int all_soa = (call - 2) >> 1, cand = (call - 2) & 1;
            bool reads_soa = false;
            const KdInstance is = pick_kd_batch_instance(t, all_soa != 0, cand != 0, &reads_soa);
            std::printf("batch %d%d %s ", all_soa, cand, traits);
            print_instance(is);
            std::printf(" %s\n", reads_soa ? "reads_soa" : "records");
        } else {  // walk KIND mesh_has_patches
            const int kind = 1 + ((call - 6) >> 1), mesh_patches = (call - 6) & 1;
            std::printf("walk %d %d %s ", kind, mesh_patches, traits);
            print_instance(pick_kd_walk_instance(t, kind, mesh_patches != 0));
            std::printf("\n");
        }
    }
    for (int i = 0; i < kKdInstanceCount; ++i) {
        if (kd_instance_index(kKdInstances[i]) != i) return 1;
        std::printf("table ");
        print_instance(kKdInstances[i]);
        std::printf("\n");
    }
    return kd_instance_index({0, 0, 0, 1, 0}) == -1 && kd_instance_index({3, 1, 0, 0, 0}) == -1 ? 0 : 1;
}
