// guidance.hpp — the host-fed kernels of the guidance front end: the arithmetic either side of the solver call in the
// reference's obstacle-avoidance ROS node (class NMPC, catkin_ws/src/nmpc_ca/src/nmpc_guidance_ca1.cpp), batched:
// one thread per instance.  The arithmetic itself is ca_guidance.hpp's (pure host + device functions with a CPU harness);
// the kernels here load, call and store.  The device-resident tick is usv_guidance_tick (usvmpc.hip).
#pragma once
#include "ca_guidance.hpp"
#include "params.hpp"
#include <hip/hip_runtime.h>

namespace usv {

constexpr int GUIDANCE_BLOCK = 64; // threads per workgroup of usv_guidance_pre: one column of its LDS scratch each

struct GuidancePtrs {
    const double *vel;   // [B][2] u, v
    const double *pose;  // [B][3] nedx, nedy, psi
    const double *wp;    // [B][2*npts]
    int npts;
    const double *obs;   // [B][lmax][3] body x, y, R
    const int *nobs;     // [B]
    int lmax;
    int *k;              // [B] waypoint index (state)
    float *past_psied;   // [B] (state; float as in the node)
    double *ak, *ye;     // [B]
    int *active;         // [B]
    double *heading, *rdes, *speed; // [B] outputs of the publish side
};

// The obstacle-simulator node's simulate() (catkin_ws/src/simulation/scripts/obstacle_sim_node.py:56-81, ned_to_body
// :101-117; ca_sense_list): every world obstacle (X, Y, R) closer to the vessel than max_visible_radius is reported in the
// body frame, in list order.  The body-frame list is what obstaclesCallback of the NMPC node receives: it is written
// straight into the front end's input buffers, so a scenario sweep needs no host round trip between "sensor" and solver.
static __global__ void usv_obstacle_sim(GuidancePtrs G, const double *world, int nw, double max_radius, int B)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const double nedx = G.pose[b * 3 + 0], nedy = G.pose[b * 3 + 1], yaw = G.pose[b * 3 + 2];
    double *out = const_cast<double *>(G.obs) + (long)b * G.lmax * 3;
    const double *w = world + (long)b * nw * 3;
    const_cast<int *>(G.nobs)[b] = ca_sense_list(nedx, nedy, yaw, w, nw, max_radius, out, G.lmax);
}

static __global__ void usv_guidance_reset(GuidancePtrs G, const double *psi, int B)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    ca_reset(G.wp + (long)b * 2 * G.npts, psi[b], G.k[b], G.past_psied[b]);
}

// writes x0, stage-0 p and lh of the solver (static-obstacle mode) for instance b; GUIDANCE_BLOCK threads per workgroup (the selection's
// distances: LDS, [GUIDANCE_LMAX entries][GUIDANCE_BLOCK lanes], a lane's column is conflict-free)
static __global__ void __launch_bounds__(GUIDANCE_BLOCK) usv_guidance_pre(DevPtrs P, GuidancePtrs G)
{
    __shared__ double s_d[GUIDANCE_LMAX * GUIDANCE_BLOCK];
    const DevSpec &S = *P.spec;
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= S.B) return;
    const int K = S.K, N = S.N;
    const double u_cb = ca_fix_u(G.vel[2 * b]);
    const double v_cb = G.vel[2 * b + 1];
    const double nedx = G.pose[3 * b], nedy = G.pose[3 * b + 1], psi = G.pose[3 * b + 2];
    double *p = const_cast<double *>(P.p) + (long)b * (N + 1) * 2 * K;
    double *lh = const_cast<double *>(P.lh) + (long)b * N * K;
    // ---- obstacles
    const double *ob = G.obs + (long)b * G.lmax * 3;
    int n = G.nobs[b];
    n = n < 0 ? 0 : (n > G.lmax ? G.lmax : n);
    n = n > GUIDANCE_LMAX ? GUIDANCE_LMAX : n; // (the scratch's rows)
    ca_select_body(ob, n, K, psi, nedx, nedy, s_d + threadIdx.x, GUIDANCE_BLOCK, p, lh, nullptr);
    // ---- waypoint manager
    int k = G.k[b];
    float pp = G.past_psied[b];
    int active;
    double ak, ye;
    ca_waypoint(G.wp + (long)b * 2 * G.npts, G.npts, nedx, nedy, k, pp, active, ak, ye);
    G.k[b] = k;
    G.active[b] = active;
    if (active) {
        G.past_psied[b] = pp;
        G.ak[b] = ak;
        G.ye[b] = ye;
        ca_x0(u_cb, v_cb, ye, psi, ak, pp, nedx, nedy, const_cast<double *>(P.x0) + (long)b * CA_NX);
    }
}

static __global__ void usv_guidance_post(DevPtrs P, GuidancePtrs G)
{
    const DevSpec &S = *P.spec;
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= S.B) return;
    if (!G.active[b]) {
        G.heading[b] = 0.0; G.rdes[b] = 0.0; G.speed[b] = 0.0;
        return;
    }
    const double x1_psied = P.x[((long)b * (S.N + 1) + 1) * 8 + 4];
    ca_publish(x1_psied, G.ak[b], P.u[(long)b * S.N], G.past_psied[b], G.heading[b], G.rdes[b], G.speed[b]);
}

} // namespace usv
