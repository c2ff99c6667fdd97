// vpt_volgrid_kernel.hip.h — K3, the kernel of the `volgrid` shader (include/vpt.h: VPT_SHADER_VOLGRID): the scene's voxel-grid instances as
// heterogeneous participating media lit by its environments, by delta tracking over brick majorants (csrc/vpt_volgrid_rule.h).
//
// Design.  K2's shape (vpt_implicit_kernel.hip.h): one workgroup = one wave64 = one 8x8 pixel tile of the tile-major state; one lane owns one
// pixel for the whole launch, keeps its PCG32 stream, radiance sum and hit count in registers (HBM state is read once and written once per
// launch) and consumes the pixel's samples serially from its own stream, so results do not depend on how lanes interleave.
//
// The unit of lockstep is ONE TRACKING STEP, not a path vertex: a free flight is a chain of dependent steps - a brick crossed, a tentative
// collision drawn and tested, the next grid instance entered - whose length varies from three (a ray past every box) to thousands (a dense
// brick) between neighbouring lanes.  Every lane carries a small state machine
//     V_TRACK                          in a free flight (walk: instance, t, the flight's nearest real collision so far) -> V_COLLIDE | V_ESCAPE | V_ABORT
//     V_NEW / V_COLLIDE / V_ESCAPE / V_ABORT   wants the shading block
// and the wave alternates between rounds of VPT_K3_STEPS tracking steps for the lanes that track and the shading block, entered when
// VPT_K3_SHADE_AT lanes wait for it or nobody tracks.  A lane's own arithmetic and draws are the rule's, step for step; only the
// interleaving across lanes is the kernel's.
//
// A tracking step is stateless about the grid: it maps the lane's point to node coordinates with the density lookup's own operations,
// takes the brick that holds it, and the ray's exit from that brick from the node-space direction kept since the instance was entered.
// Nothing is carried from brick to brick, so no segment can be skipped or counted twice: t only grows, and every stretch [t, exit) is
// flown with the majorant of the brick its start lies in.  A step that rounding keeps from advancing moves on by 4e-5 of a cell.
// Every loop is bounded: a free flight by VPT_VOLGRID_MAX_STEPS (the launch then reports it through the handle's watchdog counter), a
// path by `bounces`, a lane by its samples.
//
// The records (128 bytes per grid instance) are copied into LDS at wave start, like K2's sdf_recs: they are read at every step, one
// address by all lanes that walk the same instance.  The brick tables are read from HBM with plain loads: a 96^3 grid has 1 728 bricks
// (7 KiB), they stay in L2, and neighbouring lanes read neighbouring bricks; an LDS copy would have to be made per wave for every volume
// of the scene and bounds the scene by LDS size - not built, the simpler form stays.
//
// The knobs: VPT_K3_STEPS tracking steps per round, VPT_K3_SHADE_AT waiting lanes that trigger the shading block.  Values run so far:
// K2's settled pair alone (12 / 20): 2 150 Msamples/s on the dense cloud, 3 607 on the sparse grid at 1280 x 533 x 64 spp (DESIGN.md §29,
// profiles/volgrid_measure.json).  No other pair has been measured yet; VPT_K3_WAVES 4 against 5 (vpt_launch.h) neither.
// Measured: the brick walk against one majorant per volume (VPT_VOLGRID_NO_BRICKS=1): sparse 3 607 against 2 680 Msamples/s (kept for
// that), dense 2 150 against 2 567 - a brick step pays a second point transform, three divisions and a table load.
#pragma once
#include "vpt_mesh_kernel.hip.h"   // other_light_pdf: the environment branch of sample_lights_pdf
#include "vpt_volgrid_rule.h"

// (VPT_VOLGRID_MAX_STEPS, the bound on the tracking steps of ONE free flight: include/vpt.h)
#define VPT_K3_STEPS 12      // tracking steps between two looks at the wave's state
#define VPT_K3_SHADE_AT 20   // lanes waiting for the shading block before the wave runs it

enum { V_NEW = 0, V_TRACK = 1, V_COLLIDE = 2, V_ESCAPE = 3, V_ABORT = 4, V_DONE = 5 };

// a free flight in progress
struct vg_walk {
  int   g;            // the grid instance being walked (-1: none entered yet)
  int   hit_g;        // the instance of the nearest real collision so far (-1: none)
  int   steps;
  float t, t_end;     // where the lane is in instance g, and where g's box (or the nearest collision) ends; t >= t_end: enter the next
  float tmax;         // the nearest real collision so far
  f3    dn;           // d(node coordinate) / dt of the ray in instance g
};
VPT_DEV void vg_start(vg_walk& w) { w.g = -1, w.hit_g = -1, w.steps = 0, w.t = 0, w.t_end = 0, w.tmax = VPT_FLT_MAX; }

// one tracking step of track(ray, rng) (include/vpt.h); returns the lane's next mode
VPT_DEV int vg_track_step(const DScene& sc, const volgrid_args& va, const vpt_volgrid_record* recs, f3 ro, f3 rd, rng_t& rng, vg_walk& w) {
  if (w.steps >= VPT_VOLGRID_MAX_STEPS) return V_ABORT;
  w.steps++;
  if (!(w.t < w.t_end)) {   // enter the next instance: clip the ray against its box in local space, keep the world-space parameter
    w.g++;
    if (w.g >= va.num_instances) return w.hit_g >= 0 ? V_COLLIDE : V_ESCAPE;
    const vpt_volgrid_record& rec = recs[w.g];
    float ol[3], dl[3];
    vpt_volgrid_to_local(rec.frame, ro.x, ro.y, ro.z, ol);
    vpt_volgrid_vector_to_local(rec.frame, rd.x, rd.y, rd.z, dl);
    float t0 = 0, t1 = w.tmax;
    bool  miss = rec.whd[0] <= 0 || rec.whd[1] <= 0 || rec.whd[2] <= 0;
    for (int k = 0; k < 3; k++) {
      if (dl[k] == 0) miss = miss || !(ol[k] >= 0 && ol[k] <= rec.bbox[k]);
      else {
        const float ta = (0 - ol[k]) / dl[k], tb = (rec.bbox[k] - ol[k]) / dl[k];
        t0 = fmax_(t0, fmin_(ta, tb)), t1 = fmin_(t1, fmax_(ta, tb));
      }
    }
    w.t = w.t_end = 0;
    if (!miss && t0 < t1) {
      w.t = t0, w.t_end = t1;
      w.dn = mk3(dl[0] / rec.bbox[0] * (rec.whd[0] - 1), dl[1] / rec.bbox[1] * (rec.whd[1] - 1), dl[2] / rec.bbox[2] * (rec.whd[2] - 1));
    }
    return V_TRACK;
  }
  const vpt_volgrid_record& rec = recs[w.g];
  const int nbx = vpt_volgrid_bricks(rec.whd[0]), nby = vpt_volgrid_bricks(rec.whd[1]), nbz = vpt_volgrid_bricks(rec.whd[2]);
  // the brick the lane stands in and the majorant of the stretch ahead
  float texit = w.t_end, mj;
  if (va.no_bricks) mj = va.bricks[rec.brick_offset + nbx * nby * nbz];
  else {
    float pl[3], node[3];
    const f3 p = ro + rd * w.t;
    vpt_volgrid_to_local(rec.frame, p.x, p.y, p.z, pl);
    int b[3];
    const float dn[3] = {w.dn.x, w.dn.y, w.dn.z};
    const int   nb[3] = {nbx, nby, nbz};
    for (int k = 0; k < 3; k++) {
      // (a point that rounding left a hair outside the box is clamped into it, as the lookup clamps its coordinate)
      node[k] = vpt_volgrid_node_coord(pl[k], rec.bbox[k], rec.whd[k]);
      b[k]    = vpt_volgrid_brick_of(node[k], nb[k]);
      if (dn[k] < 0 && b[k] > 0 && node[k] == (float)(b[k] * VPT_VOLGRID_BRICK)) b[k]--;   // on a brick's lower face, going down: the brick below
      if (dn[k] > 0) texit = fmin_(texit, w.t + ((float)((b[k] + 1) * VPT_VOLGRID_BRICK) - node[k]) / dn[k]);
      else if (dn[k] < 0) texit = fmin_(texit, w.t + ((float)(b[k] * VPT_VOLGRID_BRICK) - node[k]) / dn[k]);
    }
    mj = va.bricks[rec.brick_offset + b[0] + nbx * (b[1] + nby * b[2])];
  }
  if (mj > 0) {
    const float m  = mj / rec.trdepth;                         // the majorant as extinction
    const float tn = w.t + -logf(1 - rand1f(rng)) / m;
    if (tn < texit) {   // a tentative collision inside the brick: real with probability min(sigma / m, 1)
      w.t = tn;
      const f3    p     = ro + rd * tn;
      const float sigma = vpt_volgrid_density(rec, sc.voxels, p.x, p.y, p.z);
      if (rand1f(rng) < fmin_(sigma / m, 1.0f)) w.tmax = tn, w.hit_g = w.g, w.t_end = tn;   // nearer than any before: the box was clipped at tmax
      return V_TRACK;
    }
  }
  // to the brick's exit; the process is memoryless, the overshoot is discarded
  if (!(texit > w.t)) {   // rounding left the point a hair before a face it has reached: on by 4e-5 of a cell (and by an ulp of t at least)
    const float dmax = fmax_(fabs_(w.dn.x), fmax_(fabs_(w.dn.y), fabs_(w.dn.z)));
    texit = dmax > 0 ? fmin_(w.t_end, w.t + (4e-5f / dmax + w.t * 2.4e-7f)) : w.t_end;
  }
  w.t = texit;
  return V_TRACK;
}

// the light-list entries with an environment, in list order: the k-th of them
VPT_DEV int vg_env_light(const DScene& sc, int k) {
  int l = 0;
  for (; l < sc.num_lights; l++) {
    const int kind = __float_as_int(sc.light_rec[8 * l + 7].w) & 255;
    if ((kind == VPT_LIGHT_ENV_TEX || kind == VPT_LIGHT_ENV_CONST) && k-- == 0) break;
  }
  return l;
}
// sample_lights' environment branch (yocto_pathtrace.cpp:332-349) for light `light_id`
VPT_DEV f3 vg_sample_env(const DScene& sc, int light_id, float rel, f2 ruv) {
  const float4* rec = sc.light_rec + 8 * (long long)light_id;
  const float4  r6 = rec[6];
  if ((__float_as_int(rec[7].w) & 255) == VPT_LIGHT_ENV_TEX) {
    const int pick = sample_light_cdf(sc, light_id, rel);
    const int tw = __float_as_int(r6.x), th = __float_as_int(r6.y);
    f2 uv = mk2(((pick % tw) + 0.5f) / tw, ((pick / tw) + 0.5f) / th);
    return transform_direction(unpack_frame(rec[3], rec[4], rec[5]),
        mk3(cosf(uv.x * 2 * VPT_PI) * sinf(uv.y * VPT_PI), cosf(uv.y * VPT_PI), sinf(uv.x * 2 * VPT_PI) * sinf(uv.y * VPT_PI)));
  }
  return sample_sphere(ruv);
}
// sample_lights_pdf's environment branch summed over the environment lights, times 1 / their number
VPT_DEV float vg_env_pdf(const DScene& sc, int num_env, f3 position, f3 direction) {
  float sum = 0;
  for (int l = 0; l < sc.num_lights; l++) {
    const float4 r6 = sc.light_rec[8 * l + 6];
    const int    kind = __float_as_int(sc.light_rec[8 * l + 7].w) & 255;
    if (kind == VPT_LIGHT_ENV_TEX || kind == VPT_LIGHT_ENV_CONST) sum += other_light_pdf<0>(sc, l, kind, r6, position, direction, 0);
  }
  return sum * ((float)1 / (float)num_env);
}

__device__ __forceinline__ void volgrid_kernel_body(const DScene& sc, const DParams& pr, const volgrid_args& va, float4* __restrict__ image,
    int* __restrict__ hits, ulonglong2* __restrict__ rngs, const sched_cfg& sched) {
  extern __shared__ int4 lds_recs4[];
  // the records, copied once into LDS (read at every tracking step)
  {
    const int4* src = (const int4*)va.recs;
    const int   n4  = va.num_instances * (int)(sizeof(vpt_volgrid_record) / sizeof(int4));
    for (int i = threadIdx.x; i < n4; i += VPT_BLOCK) lds_recs4[i] = src[i];
  }
  __shared__ unsigned long long s_wave_start;   // the start stamp, parked in LDS (clock_ticks, vpt_math.hip.h)
  if (threadIdx.x == 0) s_wave_start = clock_ticks(blockIdx.x);
  __syncthreads();
  const vpt_volgrid_record* recs = (const vpt_volgrid_record*)lds_recs4;
  const unsigned long long  wave_start = s_wave_start;
  const int wave = sched.order ? sched.order[blockIdx.x] : (int)blockIdx.x;

  int slot = wave * VPT_BLOCK + threadIdx.x;
  if (sched.lane_slot) slot = sched.lane_slot[slot];   // a split tile or an adaptive round: the lane's state slot
  int px = 0, py = 0;
  const bool owner = slot >= 0 && slot < pr.nslots && slot_to_pixel(pr, slot, px, py);   // padding lanes own no pixel: they stay V_DONE
  if (__builtin_amdgcn_ballot_w64(owner) == 0) return;
  const int pixels   = __popcll(__builtin_amdgcn_ballot_w64(owner));   // the quorum is sized for 64 pixels: a partly filled wave scales it
  const int shade_at = max(1, (VPT_K3_SHADE_AT * pixels + 63) >> 6);

  f4    acc = mk4(0, 0, 0, 0);
  rng_t rng = {0, 0};
  if (owner) {
    float4     acc_in = image[slot];
    ulonglong2 r_in   = rngs[slot];
    acc = mk4(acc_in.x, acc_in.y, acc_in.z, acc_in.w), rng.state = r_in.x, rng.inc = r_in.y;
  }
  const vpt_camera& cam = sc.cameras[pr.camera];
  const int  nb  = pr.bounces;
  const bool mis = !pr.noimplicit_mis && va.num_env_lights > 0;

  int     mode = owner ? V_NEW : V_DONE;
  f3      ro = mk3(0, 0, 0), rd = mk3(0, 0, 1);
  f3      radiance = mk3(0, 0, 0), weight = mk3(1, 1, 1);
  float   hit = 0;
  int     bounce = 0, sample = 0, aborted = 0;
  vg_walk w;
  vg_start(w);
  unsigned long long steps = 0;

  while (true) {
    const unsigned long long tracking = __builtin_amdgcn_ballot_w64(mode == V_TRACK);
    const unsigned long long waiting  = __builtin_amdgcn_ballot_w64(mode != V_TRACK && mode != V_DONE);
    if ((tracking | waiting) == 0) break;   // every lane V_DONE

    if (tracking != 0 && __popcll(waiting) < shade_at) {
      for (int k = 0; k < VPT_K3_STEPS; k++)
        if (mode == V_TRACK) mode = vg_track_step(sc, va, recs, ro, rd, rng, w);
      continue;
    }

    // ---- shading block: the lanes that wait for it ---------------------------------------------------
    bool finish = false;
    if (mode == V_ESCAPE) {
      radiance = radiance + weight * eval_environment(sc, rd);
      steps += w.steps;
      finish = true;
    } else if (mode == V_ABORT) {   // the flight ran into its bound: the path ends with nothing added
      aborted++;
      steps += w.steps;
      finish = true;
    } else if (mode == V_COLLIDE) {
      steps += w.steps;
      const vpt_volgrid_record& rec = recs[w.hit_g];
      const f3 position = ro + rd * w.tmax, outgoing = -rd;
      const f3 albedo = mk3(rec.albedo[0], rec.albedo[1], rec.albedo[2]);
      if (bounce == 0) hit = 1;
      radiance = radiance + weight * mk3(rec.emission[0], rec.emission[1], rec.emission[2]);
      f3 incoming;
      if (!mis) {   // as sample_scattering draws: rn, then the rnl nobody reads (yocto_pathtrace.cpp:665)
        f2 rn;
        rn.x = rand1f(rng);
        rn.y = rand1f(rng);
        (void)rand1f(rng);
        incoming = sample_phasefunction(rec.g, outgoing, rn);
        weight   = weight * albedo;   // no division: f / pdf is 1 by construction
      } else {
        if (rand1f(rng) < 0.5f) {
          f2 rn;
          rn.x = rand1f(rng);
          rn.y = rand1f(rng);
          (void)rand1f(rng);
          incoming = sample_phasefunction(rec.g, outgoing, rn);
        } else {   // as sample_lights draws: ruv, rel, rl
          f2 ruv;
          ruv.x = rand1f(rng);
          ruv.y = rand1f(rng);
          const float rel = rand1f(rng);
          const float rl  = rand1f(rng);
          incoming = vg_sample_env(sc, vg_env_light(sc, sample_uniform(va.num_env_lights, rl)), rel, ruv);
        }
        const float f = eval_phasefunction(rec.g, outgoing, incoming);
        weight = weight * (albedo * (f / (0.5f * f + 0.5f * vg_env_pdf(sc, va.num_env_lights, position, incoming))));
      }
      if (is_zero3(weight) || !finite3(weight)) finish = true;
      else if (bounce > 3) {   // min(1, .): a medium of albedo 1 keeps its weight for ever (include/vpt.h: not the reference's 0.99)
        const float rr = fmin_(1.0f, max3(weight));
        if (rr < 1) {
          if (rand1f(rng) >= rr) finish = true;
          else weight = weight / rr;
        }
      }
      bounce++;
      if (bounce >= nb) finish = true;
      if (!finish) {
        ro = position, rd = incoming, mode = V_TRACK;
        vg_start(w);
      }
    }
    if (finish) {
      f4 rad = mk4(radiance.x, radiance.y, radiance.z, hit);
      if (!(isfinite(rad.x) && isfinite(rad.y) && isfinite(rad.z) && isfinite(rad.w))) rad = mk4(0, 0, 0, 0);
      acc = acc + rad;
      sample++;
      mode = V_NEW;
    }
    if (mode == V_NEW) {
      if (sample == pr.nsamples) mode = V_DONE;
      else {
        float u, v;
        if (pr.preview) {
          u = (px + 0.5f) / pr.width, v = (py + 0.5f) / pr.height;
        } else {
          u = (px + rand1f(rng)) / pr.width;
          v = (py + rand1f(rng)) / pr.height;
        }
        f2 lens;
        lens.x = rand1f(rng);
        lens.y = rand1f(rng);
        ray_t ray = eval_camera(cam, mk2(u, v), lens);
        ro = ray.o, rd = ray.d;
        radiance = mk3(0, 0, 0), weight = mk3(1, 1, 1), hit = 0;
        bounce = 0, mode = V_TRACK;
        vg_start(w);
        if (nb <= 0) mode = V_ESCAPE, weight = mk3(0, 0, 0);   // no bounce allowed: the loop body never runs (radiance 0, no hit)
      }
    }
  }

  if (aborted > 0 && va.watchdog) atomicAdd(va.watchdog, (unsigned)aborted);
  if (owner) {
    image[slot] = make_float4(acc.x, acc.y, acc.z, acc.w);
    hits[slot] += pr.nsamples;
    ulonglong2 r_out;
    r_out.x = rng.state, r_out.y = rng.inc;
    rngs[slot] = r_out;
    if (va.steps) atomicAdd(va.steps, steps);
  }
  if (sched.cost && threadIdx.x == 0) {
    unsigned long long dt = clock_ticks(__float_as_int(acc.x)) - wave_start;   // after the last sample was accumulated
    sched.cost[wave] = dt < 0xffffffffull ? (unsigned)dt : 0xffffffffu;
  }
}

// the kernel (launch bounds: vpt_launch.h; instances: vpt_k3.hip).  PILOT: the same kernel under another name, the short launch that measures
// per-wave costs when none are known yet (vpt_schedule.h), kept apart so that profiles of the render launch hold full launches only
template <bool PILOT>
__global__ void vpt_volgrid_kernel(DScene sc, DParams pr, volgrid_args va, float4* __restrict__ image, int* __restrict__ hits,
    ulonglong2* __restrict__ rngs, sched_cfg sched) {
  volgrid_kernel_body(sc, pr, va, image, hits, rngs, sched);
}
