/*
 * pt.h — C ABI of the MI355X-native path tracer (libpt.so).
 *
 * The reference (Nablax/Path-Tracer-CUDA-OpenGL) has no plugin/FFI layer: its boundary is
 * the set of CUDA kernel launches and host helpers in main.cu / utils/bvh.h.  Each entry
 * point below names the reference interface it replaces.  All functions return PT_OK (0)
 * or a PT_ERR_* code; the message of the last failure on the calling thread is returned by
 * pt_last_error().  No torch or HIP types appear in any signature: device pointers and
 * streams are passed as plain pointers.
 *
 * Threading: one pt_scene / pt_film per device; calls on different objects may come from
 * different threads.  There is no global mutable state besides the thread-local error.
 */
#ifndef PT_H
#define PT_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PT_ABI_VERSION 1

enum pt_status {
    PT_OK = 0,
    PT_ERR_INVALID = 1,   /* bad argument */
    PT_ERR_HIP = 2,       /* HIP runtime error (reference: checkCudaErrors, cuda_check.h:8-17) */
    PT_ERR_IO = 3,        /* file could not be read / written */
    PT_ERR_NOMEM = 4,
    PT_ERR_NODEVICE = 5,  /* no GPU visible: the library never falls back to the CPU */
    PT_ERR_STATE = 6      /* e.g. render before the BVH was built */
};

/* Object and material types: simulation/cuda_object.h:12-14, simulation/material.h:13-15 */
enum { PT_SPHERE = 1, PT_TRIANGLE = 3 };
enum { PT_LAMBERTIAN = 1, PT_METAL = 2, PT_DIELECTRIC = 4, PT_EMISSIVE = 8 };
/* PT_EMISSIVE (no counterpart in the reference, whose only light is its sky): albedo[3] is the
 * emitted radiance E (RGB), fuzz and ir are ignored.  A ray that hits an emissive object, from
 * either side, ends its path there: the path contributes att * E per channel (att = the path's
 * attenuation so far, (1,1,1) on a primary hit; one fp32 multiply per channel).  The hit draws no
 * random number and counts in pt_stats.rays like any other.  A path that runs out of bounces still
 * returns sky x attenuation.  Any other unknown material type absorbs (a black contribution).
 * Every component of E must be finite and in [0, PT_MAX_RADIANCE] (pt_scene_create checks it);
 * the same bound holds for the sky colours of pt_scene_set_sky.  The bound comes from the
 * sample-mode accumulator, signed 32.32 fixed point: a pixel's sum of N samples of radiance <= R
 * is exact while N * R < 2^31, so 1024 keeps 2^21 accumulated samples per pixel safe (next to the
 * "at most 2^24 - 1 accumulated samples" of PT_RENDER_ACCUMULATE, which holds for radiance <= 128). */
#define PT_MAX_RADIANCE 1024.0f
/* PT_RENDER_NEE (pt_render_opts.flags): next-event estimation, direct sampling of the emissive
 * triangles.  The reference's Lambertian scatters along n + unit vector, exactly cosine-weighted with
 * attenuation = albedo, so a light sample weighted with the Lambert BRDF albedo / pi has the blind
 * integrator's expectation; the rule below adds it to the loop and takes the same light out of the
 * scattered ray.  Without the flag nothing changes.
 * Lights: the scene's objects of type PT_TRIANGLE whose material is PT_EMISSIVE, in object-index
 *   order, nL of them (pt_scene_light_count), listed on the device by every pt_scene_build_bvh* (so
 *   after pt_scene_update_objects too) as {v0, e1 = v1 - v0, e2 = v2 - v0, E}.  Emissive spheres are
 *   not sampled; they emit when hit, as ever.
 * nL == 0: the flag changes nothing at all (image bits, RNG streams, counters; no clamp either).
 * Where: at a hit on a PT_LAMBERTIAN material, after its scatter, when the path goes on (bounces
 *   left; a path out of bounces ends with sky x attenuation and takes no light sample).
 * Draws: three more curand_uniform values of the path's stream, after the material's own: uL, ua, ub
 *   -- always, whatever the geometry tests below say.
 * Every operation below is one rounded fp32 operation, in this order (dot(a, b) = (a.x * b.x + a.y *
 * b.y) + a.z * b.z; cross(u, v) = (u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x)):
 *   k = min((int)(uL * (float)nL), nL - 1);   if (ua + ub > 1) { ua = 1 - ua; ub = 1 - ub; }
 *   ub = fminf(ub, 1 - ua);   ua = fminf(ua, 1 - ub)      (the fold's sum is a rounded one: a point it
 *   left up to 2^-24 outside the edge ua + ub = 1 moves onto it; then ua, ub >= 0 and ua + ub <= 1 hold
 *   exactly -- 1 - x is exact for x >= 0.5, and a pair of values below 0.5 needs no help)
 *   q = (v0 + ua * e1) + ub * e2;   w = q - p          (p = the hit point, the scatter ray's origin)
 *   cs = dot(n, w)   (n = the hit's normal, facing the incoming ray);   cl = |dot(cross(e1, e2), w)|;
 *   d2 = dot(w, w).   cs <= 0, cl == 0 or d2 == 0: no shadow ray, nothing added.
 *   Shadow ray (p, w), unnormalised: occluded exactly when pt_trace_closest_ex(tmin = 0.001, tmax =
 *   0.999) reports a hit for it (pt_trace_occluded's definition; the light sits at t = 1, the 0.001 at
 *   either end is the reference's self-hit margin in parametric units).  It counts in pt_stats.rays
 *   and the node / box / primitive counters like any query, not in `paths`, and uses up no bounce.
 *   Unoccluded: G = ((cs * cl) * (float)nL) / (6.2831855f * (d2 * d2))   (|cross(e1, e2)| carries the
 *   light's area and 1 / pdf; an IEEE division), and per channel direct += ((att * albedo) * E) * G,
 *   att = the attenuation before this hit; a NaN channel of that product counts as 0.  `direct` is
 *   the path's own running sum, 0 at the camera.
 * No double counting: a ray scattered at a Lambertian hit (nL > 0) that lands on a sampled light (an
 *   emissive triangle) ends the path with 0 instead of att * E.  Every other emitter hit is as before:
 *   a primary hit, a hit after a metal or dielectric scatter, any hit on an emissive sphere.
 * Clamp: a finished sample contributes fminf(direct + ending term, PT_MAX_RADIANCE) per channel (one
 *   add, one fminf).  G is unbounded near a light; the clamp keeps the sample-mode accumulator exact
 *   while N * PT_MAX_RADIANCE < 2^31 and is the rule's one deliberate bias.
 * Instanced scenes list their lights on request: pt_scene_build_bvh* with PT_BVH_LIGHTS (below).
 *   Lights: the (instance, object) pairs whose object is a PT_TRIANGLE with a PT_EMISSIVE material, in
 *   flattened object order (instances in order, each contributing its mesh's emissive triangles in
 *   object order); nL is their number and does not depend on the matrices.  Each vertex (x, y, z) of
 *   the triangle goes to the world through the instance's matrix m in fp64: row r gives
 *   w_r = ((m[r][0] * x + m[r][1] * y) + m[r][2] * z) + m[r][3], m, x, y, z converted to double, one
 *   rounded fp64 operation each in that order, no contraction; w_r is rounded to fp32 once.  Then
 *   e1 = v1' - v0' and e2 = v2' - v0' in fp32 of the rounded vertices, and E is the material's albedo.
 *   An identity matrix therefore gives the flat scene's record bit for bit.  Emission is two-sided and
 *   cl an absolute value, so a mirrored instance (det < 0) needs no special case.  Everything else of
 *   the rule is unchanged: p and n are the instanced hit's world-space point and normal; "a sampled
 *   light" hit by a scatter ray is an emissive triangle of any instance; the shadow ray is an instanced
 *   closest-hit query over the same interval, which like every instanced result equals the flattened
 *   scene's within the documented tolerance (bit for bit for identity instances).  The records follow
 *   pt_scene_update_instances: every build with the bit writes them from the current matrices with the
 *   same device code, the top-level-only rebuild included (no allocation there either), so a rebuilt
 *   scene's list is a fresh scene's bit for bit.  64 B per record.
 * Scope: PT_KERNEL_WIDE / PT_KERNEL_DEFAULT on flat scenes and on instanced scenes whose last build
 *   had PT_BVH_LIGHTS, PT_KERNEL_SIMPLE on flat scenes; both RNG modes, with PT_RENDER_ACCUMULATE,
 *   partitioned films and every output format.  With the flag, PT_KERNEL_WAVEFRONT and an instanced
 *   scene whose last build did not have PT_BVH_LIGHTS are PT_ERR_INVALID and nothing is rendered. */
#define PT_RENDER_NEE 4
/* PT_RENDER_MIS (pt_render_opts.flags): next-event estimation with multiple importance sampling
 * (balance heuristic) between the light sample and the Lambertian scatter ray.  It implies
 * PT_RENDER_NEE, whether or not that bit is set.  G above is unbounded next to a light and only the
 * clamp guards it; here both ways of reaching a sampled light -- the light sample, and the scatter ray
 * that happens to land on it -- stay in the estimator, each weighted with its own pdf over the sum of
 * the two, so every light term is bounded and the singular G is gone instead of clipped.  No new ray,
 * no new draw.  Without the bit nothing changes (PT_RENDER_NEE frames included).
 * Everything of the PT_RENDER_NEE rule stays: the light list, where the rule applies (a PT_LAMBERTIAN
 * hit, after its scatter, bounces left, nL > 0), the draws uL, ua, ub, k, the fold and its two fminf,
 * q, w, cs, cl, d2, the three rejections, the shadow ray over [0.001, 0.999), the counters, and the final
 * fminf(direct + ending term, PT_MAX_RADIANCE) per sample.  Two things change.  Every operation is one
 * rounded fp32 operation in the written order, dot and cross as above, sqrtf and / correctly rounded:
 * The light sample's weight replaces G.  For an unoccluded sample:
 *   len = sqrtf(d2)
 *   pl  = ((2 * d2) * len) / ((float)nL * cl)      (the light sample's pdf per solid angle: 1 / nL, uniform
 *                                                  on the triangle of area |cross(e1, e2)| / 2)
 *   pb  = cs / (3.1415927f * len)                  (the Lambertian scatter's pdf of the same direction)
 *   wl  = pb / (pl + pb)
 *   direct += ((att * albedo) * E) * wl            per channel; a NaN channel counts as 0
 *   ((albedo / pi) * E * cos / pl, the light sample's estimate, times its balance weight pl / (pl + pb).)
 * The scatter ray carries its pdf.  At the same hit, whatever the rejections say, with n the hit's
 *   normal and d the scatter ray's unnormalised direction:
 *   pbs = fmaxf(dot(n, d), 0) / (3.1415927f * sqrtf(dot(d, d)))
 * A sampled light hit by that scatter ray is weighted, not zeroed.  With t the hit's parameter and e1,
 *   e2 the hit triangle's light-record edges:
 *   wv  = t * d   (per component);   D2 = dot(wv, wv);   L = sqrtf(D2)
 *   clh = |dot(cross(e1, e2), wv)|
 *   pls = ((2 * D2) * L) / ((float)nL * clh)
 *   wb  = pbs / (pls + pbs)
 *   ending term = (att * E) * wb                   per channel; a NaN channel counts as 0
 *   Every other emitter hit is as before, with weight 1: a primary hit, a hit after a metal or
 *   dielectric scatter, any hit on an emissive sphere.
 * Consequences: wl and wb lie in [0, 1] (pb, pbs >= 0 and pl, pls > 0 or NaN; a NaN weight's term is 0),
 *   so every light term is at most (att * albedo) * E per channel, and no sample clamps in a scene
 *   with max E / (1 - max Lambertian albedo) < PT_MAX_RADIANCE (both lit presets: 17 / 0.27).  The clamp
 *   stays: the sample-mode accumulator's promise needs it whatever the scene.  A PT_RENDER_MIS frame
 *   draws the same random numbers and traces the same rays as the PT_RENDER_NEE frame of the same
 *   arguments: the streams, pt_stats.rays, paths and the work counters are identical, only the pixel
 *   values differ.
 * Instanced scenes built with PT_BVH_LIGHTS: the light list is PT_RENDER_NEE's; e1, e2 of a sampled
 *   light hit by the scatter ray are those of the hit (instance, triangle)'s own record.
 * Scope: PT_RENDER_NEE's.  With the bit, PT_KERNEL_WAVEFRONT and an instanced scene whose last build did
 *   not have PT_BVH_LIGHTS are PT_ERR_INVALID (the message names PT_RENDER_MIS) and nothing is rendered.
 *   nL == 0: the bit changes nothing at all. */
#define PT_RENDER_MIS 8

/* One scene object, the reference's CudaObj (cuda_object.h:16-123) without device pointers.
 * sphere: v[0..2] = centre, v[3] = radius (negative radius = hollow sphere, as in RTIOW)
 * triangle: v[0..2], v[3..5], v[6..8] = vertices v0, v1, v2 (one CudaObj per triangle). */
typedef struct { int32_t type; int32_t mat; float v[9]; } pt_object;

/* Material (material.h:17-68) in its constructed state: fuzz already clamped to <= 1. */
typedef struct { int32_t type; float albedo[3]; float fuzz; float ir; } pt_material;

/* camera (camera.h:10-76) after its host constructor ran (see pt_camera_make). */
typedef struct {
    float origin[3], lower_left[3], horizontal[3], vertical[3];
    float right[3], up[3], front[3];
    float focus_dist, lens_radius, time0, time1;
} pt_camera;

typedef struct { float o[3]; float d[3]; } pt_ray;                       /* simulation/ray.h */
typedef struct { int32_t hit, obj, mat, front_face; float t, p[3], n[3]; } pt_hit; /* hit_record.h:12-25 */
/* BVH node in the reference's layout (utils/bvh_node.h:8-17): internal nodes [0, n-2], root 0,
 * leaves [n-1, 2n-2]; objid = -1 for internal nodes. */
typedef struct { int32_t left, right, parent, objid; float bmin[3], bmax[3]; } pt_bvh_node;

/* Work counters of one pt_render / pt_trace_closest call (counted in-kernel). */
typedef struct {
    uint64_t rays;          /* closest-hit queries: primary + every bounce */
    uint64_t node_visits;   /* internal BVH nodes popped (each = 2 child-box tests) */
    uint64_t box_tests;
    uint64_t tri_tests;
    uint64_t sphere_tests;
    uint64_t paths;         /* camera samples */
    double kernel_ms;       /* device time of the render/trace kernel(s), HIP events */
    uint64_t algo_bytes;    /* 56*node_visits + 40*tri_tests + 20*sphere_tests */
} pt_stats;

/* A complete host-side scene description (objects, materials, camera, frame settings). */
typedef struct {
    pt_object* objects; int64_t n_objects;
    pt_material* materials; int64_t n_materials;
    pt_camera camera;
    int32_t width, height, spp, max_depth;
    char name[64];
} pt_scene_desc;

/* Instancing.  An instance places mesh `mesh` (a range of objects, in object
 * space) in the world by the affine transform world = m * (object, 1), m row-major 3 x 4. */
typedef struct { float m[12]; int32_t mesh; int32_t reserved; } pt_instance;
/* An instanced scene description (pt_preset_instanced): meshes = object ranges
 * [mesh_first[i], mesh_first[i] + mesh_count[i]) of `objects`. */
typedef struct {
    pt_object* objects; int64_t n_objects;
    int64_t* mesh_first; int64_t* mesh_count; int32_t n_meshes;
    pt_instance* instances; int64_t n_instances;
    pt_material* materials; int64_t n_materials;
    pt_camera camera;
    int32_t width, height, spp, max_depth;
    char name[64];
} pt_instanced_desc;

typedef struct pt_scene pt_scene;   /* device-resident objects, materials, LBVH */
typedef struct pt_film pt_film;     /* device-resident per-pixel RNG streams for a set of rows */

const char* pt_last_error(void);
int pt_abi_version(void);
int pt_device_count(int* count);

/* ---------------------------------------------------------------- host-side surface (no GPU) */
/* camera host ctor, camera.h:12-39 */
int pt_camera_make(const float from[3], const float at[3], float vfov_deg, float aspect,
                   float aperture, float focus_dist, float time0, float time1, pt_camera* out);
/* camera::processKeyboard, camera.h:41-56 (dir: 0 FORWARD 1 BACKWARD 2 LEFT 3 RIGHT 4 UP 5 DOWN) */
int pt_camera_move(pt_camera* cam, int dir, float delta_time);
/* Scene builders.  name: "triangle_world" (main.cu:119-196, the reference default),
 * "random_world" (main.cu:198-256), "test_world" (main.cu:57-117), "rtiow" (C1),
 * "cornell" (C2), "bunny_cornell" (C3), "bunny_field" (C5), "bunny_field_x4" (C5 at 4x the
 * triangles: 840 half-size bunnies, an HBM-resident stress case).  models_dir holds
 * cornellbox/<part>.obj and bunny/bunny.obj.  width/height <= 0 keep the preset's frame.
 * "cornell_lit" / "bunny_cornell_lit": "cornell" / "bunny_cornell" bit for bit (objects, camera, frame)
 * except that the lamp's triangles (light.obj) use a PT_EMISSIVE material of radiance (17, 12, 4),
 * appended after the box's three materials; they are meant for a black sky (pt_preset_sky). */
int pt_preset_scene(const char* name, const char* models_dir, int width, int height, pt_scene_desc* out);
/* The sky a preset is meant to be rendered under (pt_scene_set_sky's arguments): black for the
 * "_lit" presets, the reference's gradient (1,1,1) -> (0.5,0.7,1) for every other known name,
 * PT_ERR_INVALID for an unknown one.  (A call of its own: the descriptor structs are allocated by
 * the caller and keep their size under ABI version 1.) */
int pt_preset_sky(const char* name, float horizon[3], float zenith[3]);
void pt_scene_desc_free(pt_scene_desc* desc);
/* The instanced form of a preset: "bunny_field" (C5: the Cornell box once and the bunny mesh,
 * scaled x250 in object space, placed 210 times by translations -- the same grid, order and frame
 * as pt_preset_scene's flattened 1,043,312 triangles), "bunny_cornell" (box + one bunny), "cornell"
 * (the box alone), and the "_lit" forms of the last two (pt_preset_scene).  The box is instance 0
 * with the identity transform. */
int pt_preset_instanced(const char* name, const char* models_dir, int width, int height, pt_instanced_desc* out);
void pt_instanced_desc_free(pt_instanced_desc* desc);
/* OBJ mesh -> triangle objects (objl::Loader::LoadFile, OBJ_Loader.hpp:426-708, flattened to
 * one pt_object per triangle); v' = v * scale + translate.  *out is freed with pt_free. */
int pt_load_obj(const char* path, float scale, const float translate[3], int32_t mat,
                pt_object** out, int64_t* count);
void pt_free(void* p);
/* Morton keys (code << 32 | objID), stable-sorted by code: morton::computeMortonOnHost,
 * morton_code.h:64-75.  include_origin=1 seeds the scene box with the zero box (main.cu:122). */
int pt_morton_keys(const pt_object* objs, int64_t n, int include_origin, uint64_t* keys);
/* PngImage::saveColor + write (png_image.h:24-37; main.cu:477-484): rgb is row-major with
 * row 0 = bottom (as the render kernel writes it); rows are flipped on output. */
int pt_write_png(const char* path, const float* rgb, int width, int height);
/* Quantise exactly like saveColor: (uint8)(clamp(c, 0, 0.999) * 256), alpha 255, row flip. */
int pt_quantize_rgba8(const float* rgb, int width, int height, uint8_t* rgba);
/* PngImage::write of an already quantised frame (pt_render_ex with PT_OUT_RGBA8): rgba is
 * row-major with row 0 = bottom, flipped on output like pt_write_png. */
int pt_write_png_rgba8(const char* path, const uint8_t* rgba, int width, int height);

/* ---------------------------------------------------------------- device (MI355X, gfx950) */
/* Replaces the scene upload of generate*WorldOnHost (main.cu:173-192: cudaMalloc/cudaMemcpy,
 * copyObjMatsToDevice, one copyTrianglesToDevice<<<1,1>>> per triangle). */
int pt_scene_create(int device, const pt_object* objs, int64_t n_objects,
                    const pt_material* mats, int64_t n_materials, pt_scene** out);
/* The scene's sky: a ray that leaves the scene returns ((1 - t) * horizon + t * zenith) * attenuation
 * with t = 0.5 * (unit direction's y + 1), in the reference's operation order (main.cu:34-36).  A new
 * scene, flat or instanced, has the reference's sky, horizon (1,1,1) and zenith (0.5,0.7,1), and
 * renders exactly as it did before this call existed; setting those values gives the same bits.
 * The hierarchy is not touched (no rebuild).  The colours travel by value with each render's launch:
 * the call takes effect for renders enqueued after it, and a frame in flight keeps the sky it was
 * enqueued with.  PT_ERR_INVALID, and the sky left as it was, for a NULL argument or a component
 * that is not finite, negative or above PT_MAX_RADIANCE. */
int pt_scene_set_sky(pt_scene* scene, const float horizon[3], const float zenith[3]);
/* Replaces lbvh::buildBVH (bvh.h:132-145), entirely on the device: scene box, Morton codes
 * (morton_code.h:19-45), a stable radix sort by code (the reference's host std::stable_sort,
 * morton_code.h:64-75), leaf records, Karras hierarchy (bvh.h:17-115), bottom-up refit with
 * tight internal boxes (growBBox, bvh.h:117-130).  flags: PT_BVH_ORIGIN_BOUNDS (default
 * behaviour of the reference: the Morton bounds contain the origin, main.cu:122);
 * PT_BVH_HOST_KEYS computes and sorts the keys on the host instead (identical result; A/B). */
#define PT_BVH_ORIGIN_BOUNDS 1
#define PT_BVH_HOST_KEYS 2
/* PT_BVH_WIDE_DEVICE: also build the wide kernel's compressed 8-wide tree, on the device, in the
 * same call (top-down SAH + collapse, a few milliseconds even at a million primitives; for
 * dynamic scenes rebuilt every frame).  Without it PT_KERNEL_WIDE builds the tree at first use on
 * the host (binned SAH, slower to build; PT_WIDE_BUILD=device selects the device build there
 * too; after pt_scene_update_objects the device build is the default).  Either tree gives the
 * same images.  On an instanced scene the flag means "lay the scene out for instance updates"
 * (pt_scene_update_instances). */
#define PT_BVH_WIDE_DEVICE 4
/* PT_BVH_LIGHTS: on an instanced scene, list the sampled lights of PT_RENDER_NEE / PT_RENDER_MIS in
 * world space, one 64-byte record per (instance, emissive triangle of its mesh) -- the rule is stated
 * at PT_RENDER_NEE.  Opt-in, because a scene that never samples lights should not pay for the list.
 * The bit holds for that build only: a later build without it lists none (pt_scene_light_count is 0
 * again and the render flags are refused as before).  It composes with PT_BVH_WIDE_DEVICE: the
 * top-level-only rebuild after pt_scene_update_instances writes the list from tables the full build
 * made, without allocating; when the last full build did not have the bit, the first build that asks for
 * it is the full one.  On a flat scene it is ignored: flat builds list their lights as ever. */
#define PT_BVH_LIGHTS 8
int pt_scene_build_bvh(pt_scene* scene, int flags);
/* pt_scene_build_bvh with its device work enqueued on `stream` (a hipStream_t, NULL = the null
 * stream) instead of the null stream; returns when the build is complete (the tree depth is read
 * back to pick the traversal kernel). */
int pt_scene_build_bvh_ex(pt_scene* scene, int flags, void* stream);
/* An instanced scene (the reference has none: its MeshLoader is a stub,
 * mesh_loader.h:9-16, and every triangle is its own object with its own cudaMalloc, main.cu:182-190).
 * Each mesh is stored once, in object space; pt_scene_build_bvh builds a two-level tree: one
 * bottom-level 8-wide tree per mesh and a top-level tree over the instances' world boxes, all in
 * one node array.  Rays enter an instance transformed by the inverse of its matrix (the hit's t is
 * the same parameter in both spaces); normals return by the inverse transpose.  Renders and traces
 * use the wide kernel only (PT_KERNEL_WIDE or PT_KERNEL_DEFAULT).  Because the ray is transformed,
 * results equal the flattened scene's within floating-point tolerance (tests/test_gpu_instancing.py
 * states it), not bit for bit; ties between equal t are decided by (instance, primitive).  Hit
 * records report obj = the object's index in the flattened order (instances in order, each
 * contributing its mesh's objects).
 * Handedness: front_face is decided in object space, by the mesh's own winding (a triangle's
 * (v1 - v0) x (v2 - v0), a sphere's (p - c) / r), whatever the matrix.  So a mirrored instance
 * (det of m's 3 x 3 part < 0) keeps its mesh's front side, and the flattened scene it equals is the
 * one with v1 and v2 of each of its triangles swapped: a triangle transformed vertex by vertex has
 * the normal det * A^-T (e1 x e2), the opposite side for det < 0, which would turn a dielectric
 * inside out.  Against the plainly flattened vertices a mirrored instance returns the same t, p and
 * n with front_face inverted on its triangles (tests/test_gpu_instance_affine.py pins the rule). */
int pt_scene_create_instanced(int device, const pt_object* objs, int64_t n_objects, const int64_t* mesh_first,
                              const int64_t* mesh_count, int n_meshes, const pt_instance* instances, int64_t n_instances,
                              const pt_material* mats, int64_t n_materials, pt_scene** out);
/* Dynamic scenes (per-frame rebuild): overwrite objects [first, first + n)
 * (host array; same validation as pt_scene_create) and mark the hierarchy stale -- rendering or
 * tracing fails with PT_ERR_STATE until pt_scene_build_bvh runs again.  A rebuild reuses every
 * device buffer of the previous build (no allocation, no device-wide synchronisation).  The
 * reference has no counterpart: it builds once (main.cu:122-128 / bvh.h:132-145). */
int pt_scene_update_objects(pt_scene* scene, const pt_object* objs, int64_t first, int64_t n);
/* Moving instances (rigid animation of an instanced scene): overwrite the transforms of instances
 * [first, first + n) from a host array and mark the hierarchy stale -- rendering, tracing and
 * occlusion queries fail with PT_ERR_STATE until pt_scene_build_bvh / _ex runs again.  PT_ERR_INVALID
 * (and the scene left exactly as it was) for a scene that is not instanced, a range outside
 * [0, n_instances], a NULL array with n > 0, an instances[i].mesh different from the instance's
 * current mesh (the flattened object numbering and the hit key depend on it: create a new scene), a
 * non-finite matrix entry, or a singular matrix (|det| <= 1e-30 or not finite, the build's rule; the
 * message names the instance).  n == 0 changes nothing.
 * The builds of a scene whose instances were updated (or that was once built with
 * PT_BVH_WIDE_DEVICE, which for an instanced scene means "lay the scene out for updates"): the
 * first is the full host build, with the top level's region of the node array reserved at its upper
 * bound and the mesh trees quantised for twice the world's current reach into their object spaces;
 * every later one keeps the mesh trees, primitive and shading records and redoes only what depends
 * on the matrices -- the instances' exact world boxes and their entries' boxes on the device, on
 * the build's stream (every vertex of every instance in fp64), then the top-level 8-wide tree over the
 * entries (the device wide builder's SAH and collapse stages, one entry per leaf, written into the
 * reserved region) and its instance records; the world-to-object rows (64 B per instance) and the
 * scene scalars are computed on the host by the full build's own code, the scalars from the
 * instances' boxes read back.  No device allocation, no host tree build (pt_scene_wide_info source
 * 4; pt_scene_build_time: the device time of that work, HIP events).
 * When a mesh's new reach exceeds the reach its tree was built for, that build is the full one
 * again (source 3).  A rebuilt scene returns bit for bit the hits and frames of a fresh scene of
 * the same matrices -- as far as the primitive tests report no hit outside the primitive's box: the
 * rows and scalars are the fresh scene's, and the trees (another top level, mesh trees quantised for
 * twice the reach) only decide which boxes a ray enters.  The reference's float sphere test does
 * report such hits when r / distance falls to about 1e-4 (cancellation in its quadratic); which of
 * those are found then depends on the boxes entered, in any two builds of a scene.  A scene that was never updated builds exactly as before. */
int pt_scene_update_instances(pt_scene* scene, const pt_instance* instances, int64_t first, int64_t n);
/* nL, the number of sampled lights (PT_RENDER_NEE: the emissive triangles) the last build listed;
 * 0 for an instanced scene built without PT_BVH_LIGHTS.  PT_ERR_STATE before a build, or after an update
 * that made it stale. */
int pt_scene_light_count(pt_scene* scene, int64_t* n);
/* The light records of the last build, flat or instanced: nL x 12 floats, {v0, e1, e2, E} of each record
 * in list order, as the kernels read them.  PT_ERR_INVALID for a NULL scene, PT_ERR_STATE before a build
 * or on a stale scene; nL == 0 writes nothing and is PT_OK; a NULL `records` with nL > 0 is
 * PT_ERR_INVALID. */
int pt_scene_download_lights(pt_scene* scene, float* records);
/* Device time of the last pt_scene_build_bvh (HIP events around the build's stream work). */
int pt_scene_build_time(pt_scene* scene, double* ms);
int pt_scene_bvh_info(pt_scene* scene, int* depth, int64_t* n_nodes, int64_t* device_bytes);
/* The wide tree of the current build (0s before its first use): depth (levels), node slots,
 * build time in ms (wall time of the host build + upload, or of the device build when built at
 * first use; 0 when pt_scene_build_bvh built it -- then it is in pt_scene_build_time), source
 * (0 none, 1 host SAH, 2 device SAH or PLOC, 3 an instanced scene's full host build of both
 * levels, 4 an instanced scene's rebuild of the top level alone after pt_scene_update_instances). */
int pt_scene_wide_info(pt_scene* scene, int* depth, int64_t* node_slots, double* build_ms, int* source);
/* Download the LBVH in the reference's node layout (2n-1 nodes). */
int pt_scene_download_bvh(pt_scene* scene, pt_bvh_node* nodes);
/* Download one array of the current wide tree (the one pt_scene_wide_info describes), byte for byte as
 * the wide kernels read it.  The layouts are the ones host/pt_wide8.cpp documents and pt_wide8.hpp
 * sizes (node slots of kW8NodeDwords dwords, 12-dword primitive records, 8-float box records, the
 * instance rows of pt_instancing.hpp); n = the scene's objects:
 *   PT_WIDE_NODES       the node slots pt_scene_wide_info reports, from the root (slot 0) on
 *   PT_WIDE_PRIMS       n x 12 dwords, the primitive records in the tree's leaf order {v0, rank}{v1, .}{v2, .}
 *                       (an instanced scene: every mesh's records, mesh after mesh)
 *   PT_WIDE_SHADE       n x 12 dwords, the shading records by reference rank (instanced: by shading index)
 *   PT_WIDE_BOXES       n x 8 floats, the exact triangle boxes by reference rank (flat scenes)
 *   PT_WIDE_RANKS       n dwords, LBVH leaf k -> its reference rank (flat scenes)
 *   PT_WIDE_EDGE_PRIMS  n x 12 dwords, PT_WIDE_PRIMS in edge form {v0, .}{v1 - v0, .}{v2 - v0, .}: only a
 *                       flat scene that never held a sphere has it
 *   PT_WIDE_INSTANCES   16 floats per instance {world-to-object rows, objBase, class}: instanced scenes
 * *bytes (when not NULL) is always set to the array's size, 0 on an error.  out == NULL asks for the
 * size only; otherwise `capacity` bytes may be written: a capacity below the size is PT_ERR_INVALID
 * and nothing is written.  An array this scene does not have has 0 bytes and is PT_OK.  PT_ERR_INVALID
 * for a NULL scene, an unknown array or a negative capacity; PT_ERR_STATE before a build or on a
 * scene made stale by an update.  Like a query with PT_KERNEL_WIDE, the call builds the wide tree
 * when the current build has none yet.  It launches nothing: it waits for the device and copies. */
enum { PT_WIDE_NODES = 0, PT_WIDE_PRIMS = 1, PT_WIDE_SHADE = 2, PT_WIDE_BOXES = 3,
       PT_WIDE_RANKS = 4, PT_WIDE_EDGE_PRIMS = 5, PT_WIDE_INSTANCES = 6 };
int pt_scene_download_wide(pt_scene* scene, int array, void* out, int64_t capacity, int64_t* bytes);
/* RenderManager::hitBvh (render_manager.h:86-135) over a batch of rays, t in [tmin, tmax).
 * rays/hits are host pointers.
 *
 * The contract of the five ray-query entry points (pt_trace_closest, _ex, _device, pt_trace_occluded,
 * _device) on degenerate input (tests/test_gpu_degenerate_rays.py):
 * 1. Rays.  Any bit pattern in o and d is legal: NaN (quiet or signalling), infinities, zero and
 *    denormal directions, magnitudes that overflow the primitive tests.  A query never fails, never
 *    trips the traversal guard (PT_ERR_STATE) and always ends; a ray's result does not depend on the
 *    other rays of its batch.
 * 2. The rule.  The result is the reference's (RenderManager::hitBvh with CudaObj::hit, in its own
 *    fp32 operation order) with one change: a candidate whose t is NaN is not a hit.  The reference
 *    accepts such a candidate by accident of its comparison forms (every rejection is a comparison,
 *    and a NaN fails them all), keeps the NaN as its closest distance -- after which every box passes
 *    and every later candidate replaces the record -- and returns a record of NaNs; the kernels here
 *    have always rejected it (their accept test is t >= 0), at no cost.  Consequences: a ray with a
 *    NaN in any component of o or d misses everything (NaN * 0 is NaN, so the NaN reaches the t of
 *    every triangle and sphere test; the same after an instance's transform) and gets the miss
 *    record {0, -1, -1, 0, 0...}; so does the all-zero direction.  Infinite values are not special:
 *    t = +inf is a hit when the reference's arithmetic says so (a sphere root of a denormal or
 *    overflowing direction with tmax = +inf), with the p and n its arithmetic gives.  A scene of one
 *    primitive has no box test in the reference, so such a hit counts there whatever the box.
 * 3. Interval.  tmin must be >= 0 and not NaN (-0.0 counts as 0), and the scalar tmax must not be
 *    NaN: otherwise PT_ERR_INVALID before anything is launched, with hits / occluded and stats left
 *    untouched and a message "<function>: tmin must be >= 0 and not NaN" or "<function>: tmax must
 *    not be NaN".  (A negative tmin would ask for hits behind the origin, which the kernels' accept
 *    test excludes.)  tmax < tmin is legal: an empty interval, every ray misses -- a negative tmax
 *    and a scene of one primitive included.  Where ray_tmax is given the scalar tmax is ignored,
 *    whatever it holds, and a ray_tmax[i] that is NaN counts as +inf, no upper bound for that ray
 *    (it cannot be checked without a pass over device memory). */
int pt_trace_closest(pt_scene* scene, const pt_ray* rays, int64_t n, float tmin, float tmax,
                     pt_hit* hits, pt_stats* stats);
/* pt_trace_closest with a choice of tree: PT_KERNEL_WIDE traverses the compressed 8-wide tree
 * (see pt_render_ex); any other value the binary LBVH in the reference's order.  Same hits. */
int pt_trace_closest_ex(pt_scene* scene, const pt_ray* rays, int64_t n, float tmin, float tmax, int kernel,
                        pt_hit* hits, pt_stats* stats);
/* pt_trace_closest_ex on device-resident arrays (e.g. torch tensors): rays / hits are device
 * pointers, traced on `stream` (a hipStream_t, may be NULL); returns when the batch is done. */
int pt_trace_closest_device(pt_scene* scene, const pt_ray* rays, int64_t n, float tmin, float tmax, int kernel,
                            pt_hit* hits, void* stream, pt_stats* stats);
/* Visibility ("any hit") queries: occluded[i] = 1 when ray i meets any primitive with t in the
 * closest-hit query's interval, else 0 -- exactly pt_trace_closest_ex's hit flag for that ray
 * (same scene, tmin and tmax; so a triangle at exactly t == tmax does not occlude and a sphere
 * root at exactly tmax does), found without the hit record and without walking on after the
 * first blocker.  ray_tmax, when not NULL, gives each ray its own tmax (shadow rays: the distance
 * to the light) and the scalar tmax is ignored.  Degenerate rays and intervals: pt_trace_closest's
 * contract (any ray is legal and a NaN candidate is no hit; tmin < 0, a NaN tmin or a NaN scalar tmax
 * is PT_ERR_INVALID with `occluded` untouched; a NaN ray_tmax[i] counts as +inf).  kernel: PT_KERNEL_DEFAULT and PT_KERNEL_WIDE
 * traverse the compressed 8-wide tree (built at first use; the answer has no order to honour, so
 * the fast tree is the default), PT_KERNEL_SIMPLE / PT_KERNEL_WAVEFRONT the binary LBVH in the
 * reference's order (PT_ERR_INVALID on an instanced scene).  rays / ray_tmax / occluded are host
 * pointers; stats counts the work done up to each ray's first blocker. */
int pt_trace_occluded(pt_scene* scene, const pt_ray* rays, int64_t n, float tmin, float tmax,
                      const float* ray_tmax, int kernel, uint8_t* occluded, pt_stats* stats);
/* pt_trace_occluded on device-resident arrays (e.g. torch tensors): rays / ray_tmax / occluded are
 * device pointers (n rays, n floats or NULL, n bytes), traced on `stream` (a hipStream_t, may be
 * NULL); exactly n bytes are written; returns when the batch is done. */
int pt_trace_occluded_device(pt_scene* scene, const pt_ray* rays, int64_t n, float tmin, float tmax,
                             const float* ray_tmax, int kernel, uint8_t* occluded, void* stream,
                             pt_stats* stats);
/* Per-pixel XORWOW streams, initRandom (main.cu:262-269): curand_init(seed, pixel, 0, ...)
 * for every pixel of the rows this film owns.  Rows are grouped in stripes of stripe_height;
 * stripe s belongs to part (s % n_parts).  n_parts = 1 owns the whole frame. */
int pt_film_create(int device, int width, int height, int stripe_height, int n_parts, int part,
                   uint64_t seed, pt_film** out);
int pt_film_info(pt_film* film, int* n_rows, int64_t* n_pixels);
int pt_film_rows(pt_film* film, int32_t* rows);                  /* global row of each local row */
int pt_film_get_rng(pt_film* film, uint32_t* states);            /* n_pixels x {d, v0..v4} */
int pt_film_set_rng(pt_film* film, const uint32_t* states);
/* render<<<>>> (main.cu:271-294): spp samples per pixel of the film's rows, max_depth bounces.
 * Writes sqrt(mean) RGB, 3 floats per pixel, local rows in order.  out_rgb is a device
 * pointer when out_on_device != 0 (then `stream` is the hipStream_t to use, may be NULL),
 * else a host pointer.  The film's RNG streams advance, as the reference's devStates do.
 * Asynchronous when out_on_device != 0 and stats == NULL: the call enqueues the frame's kernels
 * (render, resolve, the next launch's tile order) on `stream` and returns without waiting for the
 * device; pt_film_stats() then gives the frame's counters.  With stats != NULL, or a host output,
 * the call returns when the frame is done.  Frames of one film must use one stream (or be ordered
 * by the caller): the film's buffers are reused by the next frame. */
int pt_render(pt_scene* scene, pt_film* film, const pt_camera* cam, int spp, int max_depth,
              float* out_rgb, int out_on_device, void* stream, pt_stats* stats);
/* Render options.
 * kernel: PT_KERNEL_DEFAULT (= PT_KERNEL_WIDE unless the PT_RENDER_KERNEL environment
 *   variable says "simple" or "wavefront"), PT_KERNEL_SIMPLE (ray-synchronous, the reference's loop
 *   structure, binary LBVH), PT_KERNEL_WAVEFRONT (per-lane state machine, steps chosen by wave
 *   ballots, binary LBVH, the reference's visiting order) or PT_KERNEL_WIDE (the same state
 *   machine on a compressed 8-wide SAH tree built on the host at first use, nearest child first;
 *   the closest hit is chosen by (t, the reference's tie order), so the hits are the reference's).
 *   All kernels give bit-identical images for a given rng mode.
 * rng: PT_RNG_COMPAT (default): the reference's semantics -- one cuRAND-XORWOW stream per
 *   pixel, curand_init(seed, pixel, 0), samples consumed in order and kept across calls like
 *   the reference's devStates; a pixel's samples are inherently sequential.
 *   PT_RNG_SAMPLE: one XORWOW stream per pixel-sample (the reference's generator and
 *   curand_uniform mapping), its state seeded by one Philox4x32-10 block with key = film seed and
 *   counter = {sample, pixel, 0, "SAMP"}; samples are summed in blocks of `chunk` samples
 *   (0 = max(16, ceil(spp/64))), each block's fp32 sum is converted to 32.32 fixed point and the
 *   pixel's blocks are added exactly (integer atomics: the order in which blocks finish does not
 *   matter).  (pixel, block) tasks are handed to persistent waves, longest tiles first from the
 *   previous launch's costs; neither the scheduling nor the stripe partition changes the image.
 *   Limits (PT_ERR_INVALID beyond them, nothing rendered): the film's width and rows below 65536, and
 *   tiles x blocks x 64 < 2^32 - 2^26 tasks, with tiles = ceil(width / 8) * ceil(rows / 8) of the film's
 *   own rows and blocks = ceil(spp / chunk) -- raise `chunk` for more samples.  (The tasks come from a
 *   32-bit counter that every persistent wave pushes on by one pool of 64 after the last task; the
 *   2^26 is room for 2^20 such waves, whatever the device.  A launch of more waves than that, which
 *   no current device reaches, is PT_ERR_STATE.)
 *   Deterministic, statistically identical to the reference, not its random numbers; does not
 *   advance the film's XORWOW streams.  Needs 32 bytes of device memory per pixel
 *   ({x, y, z, rays} accumulators), whatever the spp.
 *   The wide kernel builds its tree on the host at the first render after each
 *   pt_scene_build_bvh (C3 5,000 triangles ~5 ms, C5 1.04 M ~0.8 s) unless the build was asked
 *   for PT_BVH_WIDE_DEVICE (the tree built on the device, milliseconds), or on the device at
 *   first use once the scene's objects have been updated (pt_scene_update_objects: a dynamic
 *   scene; PT_WIDE_BUILD=host / device in the environment overrides).
 * leaf_batch / shade_batch: wavefront thresholds in lanes (0 = default).
 * flags: PT_RENDER_IDENTITY_ORDER disables the longest-tile-first launch order;
 *   PT_RENDER_ACCUMULATE adds the frame to the film's running sums (progressive rendering,
 *   the headless counterpart of the reference's interactive loop renderToGL/renderBySurface,
 *   main.cu:307-340, 489-528) and outputs sqrt(all accumulated samples' sum / their count);
 *   compat mode continues the film's XORWOW streams, sample mode continues the sample index.
 *   pt_film_clear() restarts the accumulation (e.g. after pt_camera_move).  At most 2^24 - 1
 *   accumulated samples per pixel.  (Sample mode's 32.32 fixed-point sums are exact while
 *   samples x radiance < 2^31: with emitters or a sky at PT_MAX_RADIANCE = 1024, 2^21 samples.)
 *   PT_RENDER_NEE: direct light sampling of the emissive triangles (the rule above, next to
 *   PT_EMISSIVE).  PT_RENDER_MIS: the same with multiple importance sampling (implies
 *   PT_RENDER_NEE; its rule follows that one).  Any other bit is ignored.
 * out_format: PT_OUT_RGB32F (3 floats per pixel), PT_OUT_RGBA8 (4 bytes per pixel, quantised on
 *   the device exactly like PngImage::saveColor, png_image.h:24-30: (uint8)(clamp(c,0,0.999)*256),
 *   alpha 255; rows in film order, row 0 = bottom, pt_write_png_rgba8 flips them) or
 *   PT_OUT_RGBA8_SURFACE (renderBySurface's conversion, main.cu:327-331: (unsigned)(c*255) in an
 *   8-bit field).  For the 8-bit formats `out_rgb` points to n_pixels x 4 bytes. */
enum { PT_KERNEL_DEFAULT = 0, PT_KERNEL_SIMPLE = 1, PT_KERNEL_WAVEFRONT = 2, PT_KERNEL_WIDE = 3 };
enum { PT_RNG_COMPAT = 0, PT_RNG_SAMPLE = 1 };
enum { PT_OUT_RGB32F = 0, PT_OUT_RGBA8 = 1, PT_OUT_RGBA8_SURFACE = 2 };
#define PT_RENDER_IDENTITY_ORDER 1
#define PT_RENDER_ACCUMULATE 2
typedef struct {
    int32_t kernel, leaf_batch, shade_batch, flags;
    int32_t rng, chunk, out_format, reserved1;
} pt_render_opts;
int pt_render_ex(pt_scene* scene, pt_film* film, const pt_camera* cam, int spp, int max_depth,
                 float* out_rgb, int out_on_device, void* stream, const pt_render_opts* opts,
                 pt_stats* stats);
/* Work counters and kernel time of the film's last pt_render / pt_render_ex; waits for that
 * frame to finish.  Reports PT_ERR_STATE if a traversal guard tripped in it (corrupt tree). */
int pt_film_stats(pt_film* film, pt_stats* stats);
/* First-hit guide buffers ("AOVs": albedo, normal, position, depth of what each pixel sees first), the
 * input of any denoiser.  One pt_aov per pixel of the film's rows, local rows in order, three 16-byte
 * rows each.  A pixel depends on nothing else, so a partitioned film writes its rows of the full frame.
 * The pixel's ray is the camera ray through the pixel centre, in the render kernels' operation order
 * (W, H = the film's full frame; every operation one rounded fp32 operation):
 *   u = ((float)col + 0.5f) * (1.0f / W);   v = ((float)globalRow + 0.5f) * (1.0f / H)
 *   o = cam.origin;   d = ((lower_left + u * horizontal) + v * vertical) - origin
 * No random number is drawn and the lens is ignored (a thin-lens camera's AOVs are those of its lens
 * centre); the film's streams, accumulators and pt_film_stats are not touched.
 * The record is defined by the hit record h that pt_trace_closest_ex(scene, ray, tmin = 0.001, tmax =
 * +inf, PT_KERNEL_WIDE) returns for that ray -- flat and instanced scenes alike (an instanced record is
 * that query's, far-origin shift included); the 8-wide tree is built at first use, like any wide query.
 *   hit:  p = h.p, n = h.n (facing the ray), obj = h.obj, mat = h.mat,
 *         depth = h.t * sqrtf((d.x * d.x + d.y * d.y) + d.z * d.z),
 *         albedo = the material's albedo for PT_LAMBERTIAN and PT_METAL, fminf(E, 1) per channel for
 *         PT_EMISSIVE, (1, 1, 1) for PT_DIELECTRIC and any other type
 *   miss: obj = mat = -1, albedo = (1, 1, 1), n = p = 0, depth = 0
 * Execution as pt_render: `out` is a device pointer when out_on_device != 0 (16-byte aligned: the rows
 * are written and, by pt_film_denoise, read as 16-byte words; `stream` is then the hipStream_t to use, may
 * be NULL), else a host pointer; asynchronous when out_on_device != 0 and stats ==
 * NULL, otherwise the call returns when the records are written.  stats: rays = the film's pixels, paths
 * = 0, the node / box / primitive counters and kernel_ms as for a trace (the scene's query counters are
 * used: like the ray queries, calls on one scene must not overlap).
 * PT_ERR_INVALID for a NULL argument or a scene and film on different devices; PT_ERR_STATE before a
 * build or on a stale scene. */
typedef struct { float albedo[3]; float depth; float n[3]; int32_t obj; float p[3]; int32_t mat; } pt_aov;   /* 48 B */
int pt_render_aov(pt_scene* scene, pt_film* film, const pt_camera* cam, pt_aov* out, int out_on_device,
                  void* stream, pt_stats* stats);
/* An edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) guided by the AOVs, for low-spp frames.
 * rgb and out are W x H x 3 floats in film order, aov W x H records; on_device = 0: host pointers, copied
 * in and out, the call is synchronous; on_device != 0: device pointers, the passes are enqueued on
 * `stream` and the call returns without waiting.  out may equal rgb: the passes ping-pong through two
 * film-owned scratch images, allocated at first use and kept (so calls on one film use one stream, or are
 * ordered by the caller).  Only a film that owns the whole frame (n_parts == 1): a stripe would need
 * halos.  The filter is domain-agnostic; callers pass pt_render's output as it is.
 * opts: NULL means {5, 0.6f, 0.1f, 0.02f}; iterations in [0, 8] (0 is a copy), every sigma finite and
 * > 0.  PT_ERR_INVALID -- before anything is enqueued, `out` untouched -- for anything else, for a NULL
 * film, rgb, aov or out, and for a partitioned film.
 * Pass i = 0 .. iterations - 1, one kernel launch each: s = 1 << i, c = the current image (the input in
 * pass 0).  Every operation is one rounded fp32 operation in the written order (no contraction, IEEE
 * division, denormals kept); dot(a, b) = (a.x * b.x + a.y * b.y) + a.z * b.z.
 *   isa2 = 1.0f / (sigma_albedo * sigma_albedo);   sc_i = sigma_color * 2^-i (exact);
 *   isc2 = 1.0f / (sc_i * sc_i)
 * Pixel (x, y) with record P, hitP = P.obj >= 0:  acc = 0, ws = 0; taps dy = -2..2 outer, dx = -2..2
 * inner, q = (x + dx * s, y + dy * s); a tap outside the frame is skipped.
 *   h = k[|dx|] * k[|dy|], k = {0.375, 0.25, 0.0625}.  The centre tap has w = h.  Any other tap, with
 *   record Q: skipped when (Q.obj >= 0) != hitP.
 *   hitP:  wn = fmaxf(0, dot(P.n, Q.n)), then wn = wn * wn six times;  dp = Q.p - P.p;
 *          dist = fabsf(dot(P.n, dp));  xx = dist / (sigma_plane * P.depth);  wp = 1 / (1 + xx * xx)
 *   else:  wn = wp = 1
 *   da = Q.albedo - P.albedo;  wa = 1 / (1 + dot(da, da) * isa2)
 *   dc = c[q] - c[p];          wc = 1 / (1 + dot(dc, dc) * isc2)
 *   w = (((h * wn) * wp) * wa) * wc;   a tap whose w is not > 0 (0 or NaN) is skipped
 *   a kept tap:  acc.ch = acc.ch + w * c[q].ch per channel,  ws = ws + w
 * "Skipped" means not added: 0 x inf never appears.  Then out.ch = acc.ch / ws.  The centre tap is always
 * kept, so ws > 0; a NaN centre stays NaN.
 * First-hit guides see the reflector, not the reflection: what a mirror or a glass ball shows is
 * filtered with the guides of the mirror or the ball. */
typedef struct { int32_t iterations; float sigma_color, sigma_albedo, sigma_plane; int32_t reserved[4]; } pt_denoise_opts;
int pt_film_denoise(pt_film* film, const float* rgb, const pt_aov* aov, float* out, int on_device, void* stream,
                    const pt_denoise_opts* opts);
/* Temporal reprojection of the film's frame history, the temporal half of SVGF-style denoisers: the
 * colour accumulated over the earlier calls is carried into the new camera through the guides' world
 * positions, tested against the guides and blended with the new frame, so that samples survive a
 * pt_camera_move (PT_RENDER_ACCUMULATE keeps them only while the camera stands still).
 * rgb and out are W x H x 3 floats in film order, aov W x H records of the same frame, out_len NULL or W x H
 * floats (each pixel's history length); cam is the camera rgb and aov were rendered with: the film keeps it
 * by value as the next call's previous camera.  Pointers and stream as pt_film_denoise: on_device = 0: host
 * pointers, copied in and out, the call is synchronous; otherwise device pointers, one kernel launch is
 * enqueued on `stream` and the call returns without waiting (aov 16-byte aligned, as pt_render_aov's
 * device output: its rows are read as 16-byte words).  out may equal rgb (a pixel reads rgb and aov
 * only at itself).  Only a film that owns the whole frame (n_parts == 1): a stripe would need halos.  Calls on
 * one film use one stream, or are ordered by the caller.
 * The film owns two history images that take turns (taps read neighbours of the old one, so it is not updated
 * in place; they are swapped when the call is enqueued), 48 B per pixel each -- three 16-byte rows {acc.rgb,
 * len}, {n, mat}, {p, hit flag} -- allocated at first use and freed by pt_film_destroy, the previous camera and
 * a "has history" flag.  They share nothing with pt_film_denoise's scratch images: a temporal call followed by
 * a denoise call on one stream compose.  The film's streams, accumulators, pt_film_stats and
 * pt_film_accumulated are not touched, and the history is independent of pt_film_clear and pt_film_reset.
 * pt_film_temporal_reset clears the flag and enqueues nothing: the next call starts a new history.
 * The history advances when the launch is enqueued; with host pointers, when the results have been copied
 * back: a call that returns an error leaves it as it was.
 * opts: NULL means {32.0f, 0.02f, 0.9f, 0}; max_history finite and >= 1, sigma_plane finite and > 0,
 * normal_cos finite and in [-1, 1]; flag bits other than PT_TEMPORAL_LINEAR are ignored.  PT_ERR_INVALID --
 * nothing enqueued; out, out_len and the history untouched -- for anything else, for a NULL film, rgb, aov,
 * cam or out, and for a partitioned film.
 * The rule.  Every operation is one rounded fp32 operation in the written order (no contraction, IEEE
 * division, correctly rounded sqrtf, denormals kept); dot and cross as defined at PT_RENDER_NEE.  Every test
 * reads "kept only when the comparison is true": a NaN rejects.
 * Pixel (x, y) with record P and colour c:  cur = c * c per channel (PT_TEMPORAL_LINEAR: cur = c).
 * have = false when the film has no history (the first call, the first after a reset, or a history of
 * another size: a film's size is fixed, so that cannot arise through this ABI) or P.obj < 0 (a
 * miss pixel never has history: the sky carries no position).  Otherwise, with the previous camera {o =
 * origin, ll = lower_left, hor = horizontal, ver = vertical}:
 *   a = ll - o;  w = P.p - o;  cvw = cross(ver, w);  cwh = cross(w, hor);  chv = cross(hor, ver);
 *   den = dot(hor, cvw);  u = (-dot(a, cvw)) / den;  v = (-dot(a, cwh)) / den;  k = dot(a, chv) / den
 *   fx = u * (float)W - 0.5f;  fy = v * (float)H - 0.5f
 *   kept only when k > 0 && fx > -1 && fx < W && fy > -1 && fy < H   (the lens is ignored, as in pt_render_aov)
 *   x0 = floorf(fx);  y0 = floorf(fy);  tx = fx - x0;  ty = fy - y0
 *   ah = 0, al = 0, ws = 0; taps j = 0, 1 outer, i = 0, 1 inner, q = (x0 + i, y0 + j); a tap outside the frame
 *   is skipped.  wq = (i ? tx : 1 - tx) * (j ? ty : 1 - ty).  With Q the history pixel at q the tap is kept only
 *   when Q was a hit, Q.mat == P.mat, dot(P.n, Q.n) >= normal_cos,
 *   fabsf(dot(P.n, Q.p - P.p)) <= sigma_plane * P.depth,
 *   (fabsf(Q.acc.r) + fabsf(Q.acc.g)) + fabsf(Q.acc.b) < INFINITY, and wq > 0.
 *   a kept tap:  ah.ch = ah.ch + wq * Q.acc.ch per channel;  al = al + wq * Q.len;  ws = ws + wq
 *   have = ws > 0;  then h.ch = ah.ch / ws,  nh = al / ws
 * Blend:  len = have ? fminf(nh + 1, max_history) : 1;  alpha = 1 / len;
 *   acc.ch = have ? h.ch + (cur.ch - h.ch) * alpha : cur.ch;  out.ch = sqrtf(acc.ch) (PT_TEMPORAL_LINEAR:
 *   out.ch = acc.ch);  out_len = len.  The new history pixel is {acc, len} with P's n, mat, p and hit flag.
 * Consequences: the history is a mean in linear radiance (pt_render's output is its square root; averaging
 * sqrt(mean) values would darken the image).  Scenes are assumed static: there are no motion vectors, so
 * after pt_scene_update_objects, pt_scene_update_instances or pt_scene_set_sky the caller resets.  A
 * non-finite history colour is never carried forward.  max_history == 1 turns the filter off, to rounding:
 * len is 1 everywhere, and a pixel with history still evaluates h + (cur - h) * 1.  The guides are
 * those of the first hit, so pt_film_denoise's limitation on mirrors and glass applies unchanged. */
#define PT_TEMPORAL_LINEAR 1
typedef struct { float max_history, sigma_plane, normal_cos; int32_t flags; int32_t reserved[4]; } pt_temporal_opts;
int pt_film_temporal(pt_film* film, const float* rgb, const pt_aov* aov, const pt_camera* cam,
                     float* out, float* out_len, int on_device, void* stream, const pt_temporal_opts* opts);
int pt_film_temporal_reset(pt_film* film);
/* Re-initialise the film's streams to their initRandom state (asynchronous on `stream`). */
int pt_film_reset(pt_film* film, void* stream);
/* Progressive rendering: zero the film's accumulated sums (asynchronous on `stream`); the number
 * of samples per pixel accumulated so far. */
int pt_film_clear(pt_film* film, void* stream);
int pt_film_accumulated(pt_film* film, int64_t* samples);
void pt_film_destroy(pt_film* film);
void pt_scene_destroy(pt_scene* scene);   /* replaces clearWorldStates (main.cu:451-460) */

#ifdef __cplusplus
}
#endif
#endif
