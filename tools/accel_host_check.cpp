// tools/accel_host_check.cpp -- the hierarchy's host build and its check (csrc/rt_accel.cpp) in a stand-alone program, for a run
// under the host's sanitizers: random scenes of 0 .. 65536 objects with NaN, infinite, inverted and huge bounds at leafSize 1, 4
// and 8 (the build's own output must pass the check), then 200 corrupted copies of each structure (the check must refuse them and
// read nothing out of bounds).  No GPU is touched.  From the repository root:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -ffunction-sections -Wl,--gc-sections \
//         -I include -I opengl_raytracing_amd/csrc -x hip opengl_raytracing_amd/csrc/rt_accel.cpp tools/accel_host_check.cpp -o accel_host_check
//   ./accel_host_check          (prints bad=0 and returns 0)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <random>
#include "rt_accel.h"
int main() {
    std::mt19937 rng(7);
    std::uniform_real_distribution<float> U(-50.f, 50.f), R(0.1f, 2.f);
    int bad = 0;
    for (int n : {0, 1, 2, 3, 5, 64, 257, 4097, 65536}) {
        std::vector<rt_object> o((size_t)n);
        if (n) memset(o.data(), 0, o.size() * sizeof(rt_object));
        for (int i = 0; i < n; i++) {
            float c[3] = {U(rng), U(rng), U(rng)}, r = R(rng);
            for (int a = 0; a < 3; a++) { o[i].boundsMin[a] = c[a] - r; o[i].boundsMax[a] = c[a] + r; }
            if (i % 97 == 3) o[i].boundsMin[0] = NAN;
            if (i % 101 == 5) o[i].boundsMax[1] = INFINITY;
            if (i % 31 == 7) { float t = o[i].boundsMin[2]; o[i].boundsMin[2] = o[i].boundsMax[2]; o[i].boundsMax[2] = t; }
            if (i % 53 == 9) { o[i].boundsMin[0] = -3e38f; o[i].boundsMax[0] = 3e38f; }
        }
        for (int leaf : {1, 4, 8}) {
            rt_accel_desc d, in; memset(&in, 0, sizeof in); in.leafSize = leaf; const char *why = nullptr;
            if (!rt_accel_resolve_desc(&in, &d, &why)) { printf("desc refused: %s\n", why); return 1; }
            RtAccelBuild b;
            rt_accel_build(o.data(), n, d, &b);
            bool ok = rt_accel_validate(o.data(), n, leaf, b.nodes.data(), b.nodes.size(), b.order.data(), b.order.size(), b.loose.data(), b.loose.size(), &why);
            if (!ok) { printf("n=%d leaf=%d: own build refused: %s\n", n, leaf, why); bad++; }
            // corrupt every field kind once: the validator must refuse and must not read out of bounds
            for (int trial = 0; trial < 200 && !b.nodes.empty(); trial++) {
                RtAccelBuild c = b;
                size_t k = rng() % c.nodes.size();
                switch (trial % 6) {
                case 0: c.nodes[k].skip = rng(); break;
                case 1: c.nodes[k].leaf = rng(); break;
                case 2: c.order[rng() % c.order.size()] = rng(); break;
                case 3: c.nodes[k].lo[rng() % 3] = NAN; break;
                case 4: c.nodes[k].hi[rng() % 3] += 1.0f; break;
                case 5: c.nodes[k].skip = (uint32_t)k; break;
                }
                bool same = memcmp(c.nodes.data(), b.nodes.data(), c.nodes.size() * sizeof(rt_accel_node)) == 0 && c.order == b.order;
                bool v = rt_accel_validate(o.data(), n, leaf, c.nodes.data(), c.nodes.size(), c.order.data(), c.order.size(), c.loose.data(), c.loose.size(), &why);
                if (v && !same) { printf("n=%d leaf=%d trial=%d: corrupted structure accepted\n", n, leaf, trial); bad++; }
            }
        }
    }
    printf("bad=%d\n", bad);
    return bad != 0;
}
