// lattice_step_check -- wn::lattice_step (csrc/wn_internal.hpp) on the grids read from stdin, one per line:
//   den nx ny z0 nz base_range oscale post_scale z_const_mode z_const with_z_const signed_step margin_cells
// Prints "0" where it refuses the grid, else "1 step pmax slack two_mids extent(8) extent(16) extent(256) extent(512)"
// (doubles with 17 digits).  Host code only: tests/test_gpu_far_lattice.py compares it with the restatement in
// tests/_far_plan.py, from which the far route tables are derived.
#include <cstdio>

#include "wn_internal.hpp"

int main()
{
    wn::GridArgs g{};
    float oscale;
    int with_z, signed_step;
    double margin;
    while (scanf("%d %d %d %d %d %f %f %f %d %f %d %d %lf", &g.den, &g.nx, &g.ny, &g.z0, &g.nz, &g.base_range, &oscale,
                 &g.post_scale, &g.z_const_mode, &g.z_const, &with_z, &signed_step, &margin) == 13) {
        g.octave_scale = oscale;
        wn::LatticeStep ls;
        if (!wn::lattice_step(g, oscale, with_z != 0, signed_step != 0, margin, &ls)) {
            printf("0\n");
            continue;
        }
        printf("1 %.17g %.17g %.17g %d %lld %lld %lld %lld\n", ls.step, ls.pmax, ls.slack, (int)ls.two_mids(), ls.extent(8),
               ls.extent(16), ls.extent(256), ls.extent(512));
    }
    return 0;
}
