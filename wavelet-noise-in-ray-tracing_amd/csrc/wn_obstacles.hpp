// wn_obstacles.hpp -- the obstacle list of include/wnoise_bounded.h as the kernels take it: by value in the launch arguments
// (16 x 32 bytes).  It is the same for every lane, so wn::obstacle_ramp's loop reads it with scalar loads and branches on the
// kind as a wave.  Shared by wn_wavelet_bounded.hip (point lists, advection), wn_wavelet_bounded_bricks.hip (brick lists) and
// wn_perlin_bounded.hip (the Perlin field, whose ramp is the double instantiation).
#pragma once

#include "wn_internal.hpp"
#include "wnoise_bounded.h"

#include <algorithm>

namespace wn {

static_assert(WN_MAX_OBSTACLES == kMaxObstacles && sizeof(wn_obstacle) == 32, "include/wnoise_bounded.h");
static_assert(WN_OBSTACLE_SPHERE == kObstacleSphere && WN_OBSTACLE_CONTAINER == kObstacleContainer &&
                  WN_OBSTACLE_HALFSPACE == kObstacleHalfspace,
              "include/wnoise_bounded.h");

struct Obstacles {
    wn_obstacle list[WN_MAX_OBSTACLES];
    int nobs;
};

// The obstacle checks of include/wnoise_bounded.h (`entry` names the call in the message), then the list by value.
inline int obstacle_args(const wn_obstacle *obstacles_host, int nobs, const char *entry, Obstacles *o)
{
    if (const char *why = obstacle_fault(obstacles_host, nobs)) return fail(WN_ERR_INVALID, "%s: %s", entry, why);
    *o = Obstacles{};
    std::copy(obstacles_host, obstacles_host + nobs, o->list);
    o->nobs = nobs;
    return WN_OK;
}

} // namespace wn
