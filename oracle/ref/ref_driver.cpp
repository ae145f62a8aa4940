// ref_driver.cpp — runs the reference's own functions on plain arrays (TEST INFRASTRUCTURE).
//
// Built by oracle/ref/build_ref.py, twice (g++, ROCm clang++), with oracle/ref/shim.h force-included
// in front.  The includes below are main.cu's, in main.cu's order (the headers only compile in that
// order); main_extract.h holds rayTracing, initRandom, render and two one-line setup kernels, cut
// out of main.cu at build time.  This file holds no arithmetic of the path tracer: it converts the
// arrays of include/pt.h / oracle/pt_oracle.h to the reference's types, calls the reference, and
// converts back.
//
//   ref_driver IN OUT [--powf=mul|libm] [--camera-draws=isolated|shared]
//
// IN and OUT are files of named arrays (oracle/refharness.py writes and reads them):
//   "PTRF", uint32 count, then per array: uint32 name length, name, uint64 bytes, data.
// IN's array "op" names the operation:
//   morton   objects                              -> keys (computeMortonOnHost; maxBox grown from
//                                                    the zero box, as every scene builder does)
//   lbvh     objects                              -> keys, nodes (buildBVH)
//   trace    objects, rays, interval[2], brute    -> hits (hitBvh on buildBVH's tree, or hit)
//   scatter  materials, case_mat, case_ray, case_hit, tapes[k][L]
//                                                 -> ok, out_ray, atten, used (Material::scatter)
//   camera   args[k][12], move_dir[k][M], move_dt[k][M]
//                                                 -> cams[k][25], moved[k][M][25]
//   reflectance  cosine[k], ref_idx[k]            -> r[k] (rayphysics::reflectance; the powf switch's
//                                                    effect on its own)
//   render   objects, materials, camera[25], params{w, h, spp, depth, launches, seed}
//                                                 -> rgb[launches][w*h][3], states[launches][w*h][6]
//                                                    (initRandom once, then `launches` x render)
//
// The named switches (each isolates one documented deviation of the oracle):
//   --powf=mul (default)   powf(x, 5) is evaluated as ((x*x)*(x*x))*x;  --powf=libm leaves libm's.
//   --camera-draws=isolated (default)   get_ray draws its lens and time numbers from randState[0]
//       (main.cu:286): the driver runs the pixels one after another and puts pixel 0's stream back
//       after every other pixel, so only pixel 0's own camera draws disturb pixel 0.
//       --camera-draws=shared leaves the reference alone (pixels in launch order).
#include <png_image.h>
#include <ctime>
#include "cuda_check.h"
#include "camera.h"
#include "render_manager.h"
#include "material.h"
#include "bvh.h"
#include "macros.h"
#include "main_extract.h"

#include <map>

#include "../pt_oracle.h"

namespace {

using Blob = std::vector<unsigned char>;
using Arrays = std::map<std::string, Blob>;

[[noreturn]] void die(const std::string& why) {
    fprintf(stderr, "ref_driver: %s\n", why.c_str());
    exit(2);
}

Arrays readArrays(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) die(std::string("cannot read ") + path);
    char magic[4];
    uint32_t count = 0;
    if (fread(magic, 1, 4, f) != 4 || memcmp(magic, "PTRF", 4) != 0 || fread(&count, 4, 1, f) != 1) die("bad case file");
    Arrays a;
    for (uint32_t i = 0; i < count; i++) {
        uint32_t nl = 0;
        uint64_t nb = 0;
        if (fread(&nl, 4, 1, f) != 1 || nl > 256) die("bad array name");
        std::string name(nl, '\0');
        if (fread(&name[0], 1, nl, f) != nl || fread(&nb, 8, 1, f) != 1) die("bad array header");
        Blob b(nb);
        if (nb && fread(b.data(), 1, nb, f) != nb) die("short array " + name);
        a[name] = std::move(b);
    }
    fclose(f);
    return a;
}

void writeArrays(const char* path, const Arrays& a) {
    FILE* f = fopen(path, "wb");
    if (!f) die(std::string("cannot write ") + path);
    const uint32_t count = (uint32_t)a.size();
    fwrite("PTRF", 1, 4, f);
    fwrite(&count, 4, 1, f);
    for (const auto& kv : a) {
        const uint32_t nl = (uint32_t)kv.first.size();
        const uint64_t nb = kv.second.size();
        fwrite(&nl, 4, 1, f);
        fwrite(kv.first.data(), 1, nl, f);
        fwrite(&nb, 8, 1, f);
        if (nb) fwrite(kv.second.data(), 1, nb, f);
    }
    if (fclose(f) != 0) die("write failed");
}

template <class T> const T* get(const Arrays& a, const char* name, size_t* n) {
    auto it = a.find(name);
    if (it == a.end()) die(std::string("missing array ") + name);
    if (it->second.size() % sizeof(T)) die(std::string("bad size of ") + name);
    *n = it->second.size() / sizeof(T);
    return reinterpret_cast<const T*>(it->second.data());
}
template <class T> T* put(Arrays& a, const char* name, size_t n) {
    Blob& b = a[name];
    b.assign(n * sizeof(T), 0);
    return reinterpret_cast<T*>(b.data());
}

vec3 v3(const float* p) { return vec3(p[0], p[1], p[2]); }
void st3(float* p, const vec3& v) { p[0] = v.x(); p[1] = v.y(); p[2] = v.z(); }

// pt_object -> CudaObj through the reference's own constructors (which compute the boxes)
std::vector<CudaObj> makeObjects(const orc_object* o, size_t n) {
    std::vector<CudaObj> objs;
    objs.reserve(n);
    for (size_t i = 0; i < n; i++) {
        if (o[i].type == ORC_SPHERE) objs.emplace_back(v3(o[i].v), o[i].v[3], o[i].mat);
        else if (o[i].type == ORC_TRIANGLE) objs.emplace_back(v3(o[i].v), v3(o[i].v + 3), v3(o[i].v + 6), o[i].mat);
        else die("object type the reference does not have");
    }
    return objs;
}

aabb sceneBox(std::vector<CudaObj>& objs) {
    aabb maxBox;
    for (auto& o : objs) maxBox.unionBoxInPlace(o.mBoundingBox);
    return maxBox;
}

Material makeMaterial(const orc_material& m) {
    Material r;
    r.mAlbedo = v3(m.albedo);
    r.mFuzz = m.fuzz;
    r.mIr = m.ir;
    r.mType = m.type;
    return r;
}

// The world as main.cu sets it up: raw zeroed memory (no constructor, never destroyed), the two
// setup kernels, buildBVH.
struct World {
    std::vector<CudaObj> objs;
    std::vector<Material> mats;
    RenderManager* world = nullptr;
    BVHNode* bvh = nullptr;
    World(const orc_object* o, size_t no, const orc_material* m, size_t nm) : objs(makeObjects(o, no)) {
        for (size_t i = 0; i < nm; i++) mats.push_back(makeMaterial(m[i]));
        checkCudaErrors(cudaMalloc((void**)&world, sizeof(RenderManager)));
        REF_LAUNCH(copyObjMatsToDevice, 1, 1)(world, objs.data(), (int)objs.size(), mats.data(), (int)mats.size());
        if (!objs.empty()) {
            aabb maxBox = sceneBox(objs);
            lbvh::buildBVH(objs, objs.data(), maxBox, bvh);
            REF_LAUNCH(copyBVHToDevice, 1, 1)(world, bvh);
        }
    }
};

void putNodes(Arrays& out, const BVHNode* bvh, size_t n) {
    orc_node* nodes = put<orc_node>(out, "nodes", n ? 2 * n - 1 : 0);
    for (size_t i = 0; n && i < 2 * n - 1; i++) {
        nodes[i].left = bvh[i].left;
        nodes[i].right = bvh[i].right;
        nodes[i].parent = bvh[i].parent;
        nodes[i].objid = bvh[i].objID;
        st3(nodes[i].bmin, bvh[i].box.mMin);
        st3(nodes[i].bmax, bvh[i].box.mMax);
    }
}

void opMorton(const Arrays& in, Arrays& out, bool withTree) {
    size_t n;
    const orc_object* o = get<orc_object>(in, "objects", &n);
    std::vector<CudaObj> objs = makeObjects(o, n);
    aabb maxBox = sceneBox(objs);
    auto sorted = morton::computeMortonOnHost(objs, maxBox);
    uint64_t* keys = put<uint64_t>(out, "keys", n);
    for (size_t i = 0; i < n; i++) keys[i] = sorted[i].mortonCode64;
    if (withTree) {
        BVHNode* bvh = nullptr;
        if (n) lbvh::buildBVH(objs, objs.data(), maxBox, bvh);
        putNodes(out, bvh, n);
    }
}

void opTrace(const Arrays& in, Arrays& out) {
    size_t no, nr, k;
    const orc_object* o = get<orc_object>(in, "objects", &no);
    const float* rays = get<float>(in, "rays", &nr);
    const float* iv = get<float>(in, "interval", &k);
    const int32_t* brute = get<int32_t>(in, "brute", &k);
    nr /= 6;
    World w(o, no, nullptr, 0);
    orc_hit* hits = put<orc_hit>(out, "hits", nr);
    for (size_t i = 0; i < nr; i++) {
        Ray r(v3(rays + 6 * i), v3(rays + 6 * i + 3));
        hit_record rec;
        bool ok = false;
        if (no) ok = brute[0] ? w.world->hit(r, iv[0], iv[1], rec) : w.world->hitBvh(r, iv[0], iv[1], rec);
        orc_hit& h = hits[i];
        h.hit = ok ? 1 : 0;
        h.obj = -1;   // hit_record has no object id
        h.mat = ok ? rec.matID : -1;
        if (ok) {
            h.front_face = rec.front_face ? 1 : 0;
            h.t = rec.t;
            st3(h.p, rec.p);
            st3(h.n, rec.normal);
        }
    }
}

void opScatter(const Arrays& in, Arrays& out) {
    size_t nm, nc, k, nt;
    const orc_material* m = get<orc_material>(in, "materials", &nm);
    const int32_t* cm = get<int32_t>(in, "case_mat", &nc);
    const float* cr = get<float>(in, "case_ray", &k);
    const orc_hit* ch = get<orc_hit>(in, "case_hit", &k);
    const float* tapes = get<float>(in, "tapes", &nt);
    const size_t L = nc ? nt / nc : 0;
    int32_t* ok = put<int32_t>(out, "ok", nc);
    float* outRay = put<float>(out, "out_ray", nc * 6);
    float* att = put<float>(out, "atten", nc * 3);
    int32_t* used = put<int32_t>(out, "used", nc);
    for (size_t i = 0; i < nc; i++) {
        if (cm[i] < 0 || (size_t)cm[i] >= nm) die("case_mat out of range");
        Material mat = makeMaterial(m[cm[i]]);
        Ray rin(v3(cr + 6 * i), v3(cr + 6 * i + 3));
        hit_record rec;
        rec.p = v3(ch[i].p);
        rec.normal = v3(ch[i].n);
        rec.matID = ch[i].mat;
        rec.t = ch[i].t;
        rec.front_face = ch[i].front_face != 0;
        curandState st{};
        st.tape = tapes + L * i;
        st.tape_len = (int)L;
        color a;
        Ray sc{vec3(), vec3()};
        ok[i] = mat.scatter(rin, rec, a, sc, &st) ? 1 : 0;
        st3(outRay + 6 * i, sc.origin());
        st3(outRay + 6 * i + 3, sc.direction());
        st3(att + 3 * i, a);
        used[i] = st.used;
    }
}

void opReflectance(const Arrays& in, Arrays& out) {
    size_t n, k;
    const float* c = get<float>(in, "cosine", &n);
    const float* e = get<float>(in, "ref_idx", &k);
    if (k != n) die("reflectance: one ref_idx per cosine");
    float* r = put<float>(out, "r", n);
    for (size_t i = 0; i < n; i++) r[i] = rayphysics::reflectance(c[i], e[i]);
}

void storeCamera(float* c, const camera& cam) {
    st3(c, cam.mPosition);
    st3(c + 3, cam.mViewportLowLeftCorner);
    st3(c + 6, cam.mHorizontalViewportSize);
    st3(c + 9, cam.mVerticalViewportSize);
    st3(c + 12, cam.mRight);
    st3(c + 15, cam.mUp);
    st3(c + 18, cam.mFront);
    c[21] = cam.mFocusDist;
    c[22] = cam.mLensRadius;
    c[23] = cam.time0;
    c[24] = cam.time1;
}

void opCamera(const Arrays& in, Arrays& out) {
    size_t na, nd, k;
    const float* args = get<float>(in, "args", &na);
    const int32_t* dir = get<int32_t>(in, "move_dir", &nd);
    const float* dt = get<float>(in, "move_dt", &k);
    const size_t nc = na / 12, M = nc ? nd / nc : 0;
    float* cams = put<float>(out, "cams", nc * 25);
    float* moved = put<float>(out, "moved", nc * M * 25);
    for (size_t i = 0; i < nc; i++) {
        const float* a = args + 12 * i;
        camera cam(v3(a), v3(a + 3), a[6], a[7], a[8], a[9], a[10], a[11]);
        storeCamera(cams + 25 * i, cam);
        for (size_t j = 0; j < M; j++) {
            const int d = dir[i * M + j];
            if (d >= 0) cam.processKeyboard((utils::directions)d, dt[i * M + j]);
            storeCamera(moved + (i * M + j) * 25, cam);
        }
    }
}

void opRender(const Arrays& in, Arrays& out, bool isolated) {
    size_t no, nm, k;
    const orc_object* o = get<orc_object>(in, "objects", &no);
    const orc_material* m = get<orc_material>(in, "materials", &nm);
    const float* c = get<float>(in, "camera", &k);
    if (k != 25) die("camera: 25 floats");
    const int64_t* p = get<int64_t>(in, "params", &k);
    if (k != 6) die("params: w, h, spp, depth, launches, seed");
    const int w = (int)p[0], h = (int)p[1], spp = (int)p[2], depth = (int)p[3], launches = (int)p[4], seed = (int)p[5];
    const size_t npix = (size_t)w * h;
    World world(o, no, m, nm);

    camera* cam;   // as main.cu: constructed on the host, copied as bytes; here its fields are the case's
    checkCudaErrors(cudaMalloc((void**)&cam, sizeof(camera)));
    camera host(vec3(0, 0, 1), vec3(0, 0, 0), 40, 1, 0, 1, 0, 1);
    host.mPosition = v3(c);
    host.mViewportLowLeftCorner = v3(c + 3);
    host.mHorizontalViewportSize = v3(c + 6);
    host.mVerticalViewportSize = v3(c + 9);
    host.mRight = v3(c + 12);
    host.mUp = v3(c + 15);
    host.mFront = v3(c + 18);
    host.mFocusDist = c[21];
    host.mLensRadius = c[22];
    host.time0 = c[23];
    host.time1 = c[24];
    checkCudaErrors(cudaMemcpy(cam, &host, sizeof(camera), cudaMemcpyHostToDevice));

    curandState* states;
    vec3* frame;
    checkCudaErrors(cudaMalloc((void**)&states, npix * sizeof(curandState)));
    checkCudaErrors(cudaMalloc((void**)&frame, npix * sizeof(vec3)));
    // main.cu's launch shape: 8 x 8 threads, one block more than needed in each direction
    const dim3 threads(globalvar::kThreadX, globalvar::kThreadY);
    const dim3 blocks(w / globalvar::kThreadX + 1, h / globalvar::kThreadY + 1);
    REF_LAUNCH(initRandom, blocks, threads)(states, w, h, seed);

    float* rgb = put<float>(out, "rgb", (size_t)launches * npix * 3);
    uint32_t* after = put<uint32_t>(out, "states", (size_t)launches * npix * 6);
    for (int l = 0; l < launches; l++) {
        if (!isolated) {
            REF_LAUNCH(render, blocks, threads)(frame, w, h, spp, depth, cam, world.world, states);
        } else {
            ref_shim::run_grid(blocks, threads, false, [&] {
                const bool pixel0 = threadIdx.x + blockIdx.x * blockDim.x == 0 && threadIdx.y + blockIdx.y * blockDim.y == 0;
                const curandState keep = states[0];
                render(frame, w, h, spp, depth, cam, world.world, states);
                if (!pixel0) states[0] = keep;
            });
        }
        for (size_t i = 0; i < npix; i++) {
            st3(rgb + ((size_t)l * npix + i) * 3, frame[i]);
            memcpy(after + ((size_t)l * npix + i) * 6, states[i].s, 6 * sizeof(uint32_t));
        }
    }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) die("usage: ref_driver IN OUT [--powf=mul|libm] [--camera-draws=isolated|shared]");
    bool isolated = true;
    for (int i = 3; i < argc; i++) {
        const std::string a = argv[i];
        if (a == "--powf=libm") ref_shim::g_powf_libm = 1;
        else if (a == "--powf=mul") ref_shim::g_powf_libm = 0;
        else if (a == "--camera-draws=shared") isolated = false;
        else if (a == "--camera-draws=isolated") isolated = true;
        else die("unknown switch " + a);
    }
    Arrays in = readArrays(argv[1]), out;
    auto it = in.find("op");
    if (it == in.end()) die("missing array op");
    const std::string op(it->second.begin(), it->second.end());
    if (op == "morton") opMorton(in, out, false);
    else if (op == "lbvh") opMorton(in, out, true);
    else if (op == "trace") opTrace(in, out);
    else if (op == "scatter") opScatter(in, out);
    else if (op == "camera") opCamera(in, out);
    else if (op == "reflectance") opReflectance(in, out);
    else if (op == "render") opRender(in, out, isolated);
    else die("unknown op " + op);
    const char* tag = REF_COMPILER;
    Blob& b = out["compiler"];
    b.assign(tag, tag + strlen(tag));
    writeArrays(argv[2], out);
    fflush(stdout);
    _Exit(0);   // as the probe did: the reference's objects own pointers they must not free here
}
