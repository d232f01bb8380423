// deep6.cpp -- instantiates k_deep for 6 time steps per pass (kernels_deep.h).  See launchers.h.
#include "launchers.h"
#include "kernels_step4.h"
#include "kernels_step5.h"
#include "kernels_deep.h"

namespace {

template <int BC, bool MASK, bool MACRO>
struct LD {
    static void go(const MarchLaunch &g, const StepArgs &a)
    {
        hipLaunchKernelGGL((k_deep<BC, MASK, MACRO, 6, DEEP_RW, DEEP_PFD>), g.grid, g.block, 0,
                           g.stream, a, g.strips, g.seg_rows, g.nsegs, g.row_end);
    }
};

}  // namespace

bool lbk_launch_deep6(int bc, bool mask, bool macro, const MarchLaunch &g, const StepArgs &a)
{
    return lbk_dispatch<LD, false>(bc, mask, macro, g, a);
}
