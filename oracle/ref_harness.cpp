/*
 * oracle/ref_harness.cpp -- a C ABI over the reference's own classes.
 *
 * TEST INFRASTRUCTURE ONLY.  oracle/ref_build.py compiles this file together
 * with the reference's sources (copied to oracle/_ref/src with their kernel
 * launches rewritten for oracle/ref_shim) into oracle/_ref/libref.so; the
 * binding is oracle/_ref.py.  Nothing here restates the reference: every
 * function calls the reference's classes and kernels in the order its
 * WinMain does (TD/WinMain.cpp; TD/ = TEST_Dungeonrun/) and copies out what
 * they left in their buffers.
 *
 * Three things are ours, each because the reference leaves them open:
 *  - the node array a Trixel mallocs is filled with a known byte (zero for
 *    a scene) before create_kd, so that the fields create_kd never writes
 *    (a leaf's s1 / s2, an interior node's tri_index) can be told from the
 *    ones it does and are not heap garbage;
 *  - the flat kernel intersect_trixel_cuda has no launcher in the reference:
 *    it is launched here with the geometry of the reference's other
 *    per-pixel launches (TD/Camera.cu:79);
 *  - a hand-made tree is written into h_tree.h_nodes / d_nodes in place of
 *    create_kd's.
 */
#include "framework.h"
#include "framework.cuh"

// the launch indices of oracle/ref_shim/cuda_runtime.h
thread_local uint3 threadIdx = {0, 0, 0}, blockIdx = {0, 0, 0};
thread_local dim3 blockDim, gridDim;

// the reference's entry points that no header of its declares (TD/read_ply.cpp:13, TD/Trixel.cu:173)
void read_ply(const char*, T_fp**, T_uint*, kd_leaf_sort**, kd_vertex**, T_uint*, u8);
__global__ void intersect_trixel_cuda(Camera::pixel_memory*, u32, Camera::trixel_memory*, Trixel::trixel_memory*, s64);

namespace {

typedef Trixel::kd_tree::kd_tree_node ref_tree_node;

// oracle/_oracle.py NODE_DTYPE
struct node_rec {
    float x0, x1, y0, y1, z0, z1, s1, s2;
    int32_t cut_flag, is_leaf;
    int64_t tri_index, left, right, parent, l, m, r;
};
static_assert(sizeof(node_rec) == 96, "NODE_DTYPE");
static_assert(sizeof(kd_leaf_sort) == 80, "LEAF_DTYPE");  // x0 x1 y0 y1 z0 z1, sx0 sy0 sz0 sx1 sy1 sz1, tri

// oracle/_oracle.py OrcCamera
struct camera_rec {
    int32_t w, h;
    float pos[3], n[3], u[3], v[3], n_mod[3], u_mod[3], v_mod[3];
    float pix_w, pix_h;
};

void to_rec(const ref_tree_node& n, node_rec* o) {
    o->x0 = n.h_bound.x0; o->x1 = n.h_bound.x1;
    o->y0 = n.h_bound.y0; o->y1 = n.h_bound.y1;
    o->z0 = n.h_bound.z0; o->z1 = n.h_bound.z1;
    o->s1 = n.s1; o->s2 = n.s2;
    o->cut_flag = n.cut_flag; o->is_leaf = n.is_leaf;
    o->tri_index = n.tri_index; o->left = n.left_node; o->right = n.right_node; o->parent = n.parent;
    o->l = n.l; o->m = n.m; o->r = n.r;
}

void from_rec(const node_rec& r, ref_tree_node* n) {
    n->h_bound.x0 = r.x0; n->h_bound.x1 = r.x1;
    n->h_bound.y0 = r.y0; n->h_bound.y1 = r.y1;
    n->h_bound.z0 = r.z0; n->h_bound.z1 = r.z1;
    n->h_bound.tri_list_index = 0;
    n->s1 = r.s1; n->s2 = r.s2;
    n->cut_flag = r.cut_flag; n->is_leaf = (u8)r.is_leaf;
    n->tri_index = r.tri_index; n->left_node = r.left; n->right_node = r.right; n->parent = r.parent;
    n->l = r.l; n->m = r.m; n->r = r.r;
}

// Trixel(n, points, colours) as TD/WinMain.cpp:114-134 makes it; rad3 == NULL: zeros.
Trixel* make_trixel(const float* points9, const float* rad3, uint32_t ntri, Color* col, int fill = 0) {
    col->c = (u32*)calloc(ntri, sizeof(u32));
    col->rad = (Color::radiance*)calloc(ntri, sizeof(Color::radiance));
    if (rad3) memcpy(col->rad, rad3, sizeof(Color::radiance) * ntri);
    T_fp* pts = (T_fp*)calloc((size_t)ntri * 9, sizeof(T_fp));
    if (points9) memcpy(pts, points9, sizeof(T_fp) * 9 * (size_t)ntri);
    Trixel* t = new Trixel(ntri, pts, col);
    free(pts);
    memset(t->h_tree.h_nodes, fill, sizeof(ref_tree_node) * t->num_voxels);
    return t;
}

void sort_and_build(Trixel* t, const kd_leaf_sort* leafs, uint32_t ntri) {
    kd_leaf_sort* list = (kd_leaf_sort*)malloc(sizeof(kd_leaf_sort) * ntri);
    memcpy(list, leafs, sizeof(kd_leaf_sort) * ntri);
    t->set_sorted_voxels(list, ntri);  // TD/WinMain.cpp:135
    t->create_kd();                    // TD/WinMain.cpp:144
    free(list);
}

void free_trixel(Trixel* t, Color* col) {
    VEC3_CUDA<T_fp>* v[] = {&t->h_mem.d_p1, &t->h_mem.h_p1, &t->h_mem.d_edges.e1, &t->h_mem.d_edges.e2, &t->h_mem.d_n};
    for (auto* a : v) { free(a->x); free(a->y); free(a->z); }
    free(t->h_mem.d_color.c); free(t->h_mem.d_color.rad); free(t->h_mem.rotate_helper_array);
    free(t->d_mem); free(t->h_tree.h_nodes); free(t->h_tree.d_nodes); free(t->d_tree);
    free(t->d_points_init_data); free(t->h_points_init_data);
    free(col->c); free(col->rad);
    delete t;
}

void free_camera(Camera* c) {
    Camera::pixel_memory& m = c->h_mem;
    VEC3_CUDA<T_fp>* v[] = {&m.rad, &m.norm, &m.pnt, &m.rmd, &m.inv_rmd, &m.sign_rmd};
    for (auto* a : v) { free(a->x); free(a->y); free(a->z); }
    free(m.d_color.c); free(m.h_color.c); free(m.d_color.rad); free(m.h_color.rad);
    free(m.d_dist.d); free(m.d_rmi.index); free(m.h_rmi.index); free(c->d_mem);
    free(c->o_prop.rotation_help_array);
    if (c->d_voxels) {  // the last add_object's (the first one's are unreachable, as in the reference)
        Camera::voxel_memory& x = c->h_voxels;
        free(x.s1); free(x.s2); free(x.children); free(x.is_leaf); free(x.cut_flags); free(x.d_Bo);
        free(x.d_voxel_index_queue); free(c->d_voxels);
    }
    if (c->d_trixels) {
        Camera::trixel_memory& x = c->h_trixels;
        free(x.d_q.x); free(x.d_q.y); free(x.d_q.z); free(x.d_t.x); free(x.d_t.y); free(x.d_t.z); free(x.d_w);
        free(c->d_trixels);
    }
    free(c->object_list);
    delete c;
}

void put4(const VEC4<T_fp>* v, float* o) { o[0] = v->x; o[1] = v->y; o[2] = v->z; o[3] = v->w; }

}  // namespace

struct ref_scene {
    Camera* cam;
    Trixel* tri;
    Object *obj1, *obj2;
    Input* input;
    Color col;
};

extern "C" {

void ref_free(void* p) { free(p); }

// ---- read_ply on a path (TD/WinMain.cpp:93-110).  The leaf list holds boxes and
// triangle indices only: read_ply leaves the six sorted positions unset.
int ref_read_ply(const char* path, int mode, float** points9, uint32_t* ntri, kd_leaf_sort** leafs) {
    T_fp* pts = NULL;
    kd_leaf_sort* lf = NULL;
    kd_vertex* verts = NULL;
    T_uint nt = 0, nv = 0;
    read_ply(path, &pts, &nt, &lf, &verts, &nv, (u8)mode);
    *points9 = pts;
    *ntri = nt;
    *leafs = lf;
    return 0;
}

// ---- merge_sort on a list, in place (TD/Trixel.h:397)
void ref_merge_sort(kd_leaf_sort* list, uint32_t n, int key) {
    kd_leaf_sort* w = (kd_leaf_sort*)malloc(sizeof(kd_leaf_sort) * n);
    merge_sort(list, w, (T_uint)n, (u8)key);
    free(w);
}

// ---- Trixel(...), set_sorted_voxels, create_kd, then h_tree.h_nodes as NODE_DTYPE
// (`fill`: the byte the node array holds before create_kd; what two fills disagree on,
// create_kd never wrote)
int ref_build_kd(const kd_leaf_sort* leafs, uint32_t ntri, node_rec* nodes, int fill) {
    Color col;
    Trixel* t = make_trixel(NULL, NULL, ntri, &col, fill);
    sort_and_build(t, leafs, ntri);
    for (s64 i = 0; i < t->num_voxels; i++) to_rec(t->h_tree.h_nodes[i], &nodes[i]);
    free_trixel(t, &col);
    return 0;
}

// ---- Camera(...), its basis and the whole rmd plane
Camera* ref_camera_create(int32_t w, int32_t h, float f_w, float f_h, float focal, const float pos[3],
                          const float la[3], const float up[3]) {
    return new Camera(w, h, f_w, f_h, focal, pos[0], pos[1], pos[2], la[0], la[1], la[2], up[0], up[1], up[2]);
}

void ref_camera_destroy(Camera* c) { free_camera(c); }

void ref_camera_basis(const Camera* c, camera_rec* o) {
    o->w = (int32_t)c->f_prop.res.w;
    o->h = (int32_t)c->f_prop.res.h;
    const VEC3<T_fp>* src[] = {&c->o_prop.pos, &c->o_prop.n, &c->o_prop.u, &c->o_prop.v,
                               &c->o_prop.n_mod, &c->o_prop.u_mod, &c->o_prop.v_mod};
    float* dst[] = {o->pos, o->n, o->u, o->v, o->n_mod, o->u_mod, o->v_mod};
    for (int k = 0; k < 7; k++) { dst[k][0] = src[k]->x; dst[k][1] = src[k]->y; dst[k][2] = src[k]->z; }
    o->pix_w = c->f_prop.pix.w;
    o->pix_h = c->f_prop.pix.h;
}

void ref_camera_rays(const Camera* c, float* out /* [count][3] */) {
    for (u64 i = 0; i < c->f_prop.res.count; i++) {
        out[3 * i] = c->h_mem.rmd.x[i];
        out[3 * i + 1] = c->h_mem.rmd.y[i];
        out[3 * i + 2] = c->h_mem.rmd.z[i];
    }
}

// ---- the inverse square roots (TD/vector.cpp:13, TD/vector.cuh:79)
void ref_host_vector_norm_n(const float* s, int64_t n, float* out) {
    for (int64_t i = 0; i < n; i++) out[i] = vector_norm(s[i]);
}

void ref_device_inverse_sqrt_n(const float* xyz, int64_t n, float* out) {
    for (int64_t i = 0; i < n; i++) out[i] = device_inverse_sqrt(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
}

// ---- a scene, in WinMain's order (TD/WinMain.cpp:69-156): the camera, the Trixel,
// the tree (from `leafs`, or `nodes` written in place of it), two Objects added.
ref_scene* ref_scene_create(int32_t w, int32_t h, float f_w, float f_h, float focal, const float pos[3],
                            const float la[3], const float up[3], const float* points9, const float* rad3,
                            uint32_t ntri, const kd_leaf_sort* leafs, const node_rec* nodes) {
    ref_scene* s = new ref_scene();
    s->input = new Input();
    s->cam = ref_camera_create(w, h, f_w, f_h, focal, pos, la, up);
    s->tri = make_trixel(points9, rad3, ntri, &s->col);
    if (leafs) {
        sort_and_build(s->tri, leafs, ntri);
    } else {
        for (s64 i = 0; i < s->tri->num_voxels; i++) from_rec(nodes[i], &s->tri->h_tree.h_nodes[i]);
        cudaMemcpy(s->tri->h_tree.d_nodes, s->tri->h_tree.h_nodes, sizeof(ref_tree_node) * s->tri->num_voxels,
                   cudaMemcpyHostToDevice);  // as create_kd ends (TD/Trixel.h:380)
    }
    s->obj1 = new Object(s->tri);
    s->obj2 = new Object(s->tri);
    s->cam->add_object(s->obj1);
    s->cam->add_object(s->obj2);
    return s;
}

void ref_scene_destroy(ref_scene* s) {
    free_camera(s->cam);
    free_trixel(s->tri, &s->col);
    delete s;  // (the Objects' quaternions and the Input stay, as in the reference)
}

// ---- rot_m, host and device, from 12 floats (rows x, y, z: i j k w)
void ref_scene_set_xform(ref_scene* s, const float x[12]) {
    Quaternion* q = s->obj1->quat;
    VEC4<T_fp>* rows[] = {q->rot_m->x, q->rot_m->y, q->rot_m->z};
    for (int r = 0; r < 3; r++) *rows[r] = VEC4<T_fp>(x[4 * r], x[4 * r + 1], x[4 * r + 2], x[4 * r + 3]);
    q->set_device_rotation(q->rot_m);  // TD/Quaternion.cu:21: the rows, w included
}

// ---- one frame of the loop (TD/WinMain.cpp:212-237).  mode 0: Object::render; 1: the
// flat kernel.  hit [n], aov [10][n] (d, pnt.xyz, norm.xyz, rad.rgb) and `shown`
// (h_color.c, what StretchDIBits gets) are read after color_pixels(PHONG_COLOR_TAG);
// `clean` is h_color.c after color_pixels(SET_COLOR_TAG).
void ref_scene_frame(ref_scene* s, int mode, int64_t* hit, float* aov, uint32_t* shown, uint32_t* clean) {
    Camera* c = s->cam;
    const u64 n = c->f_prop.res.count;
    if (mode == 0) {
        s->obj1->render(c);
    } else {
        REF_LAUNCH(intersect_trixel_cuda, 1 + ((u32)n / BLOCK_SIZE), BLOCK_SIZE)
        (c->d_mem, (u32)s->tri->num_trixels, c->d_trixels, (Trixel::trixel_memory*)s->tri->d_mem, (s64)n);
    }
    c->color_pixels(PHONG_COLOR_TAG);
    const Camera::pixel_memory& m = c->h_mem;
    memcpy(hit, m.d_rmi.index, sizeof(s64) * n);
    memcpy(aov, m.d_dist.d, sizeof(float) * n);
    const T_fp* planes[] = {m.pnt.x, m.pnt.y, m.pnt.z, m.norm.x, m.norm.y, m.norm.z};
    for (int k = 0; k < 6; k++) memcpy(aov + (1 + k) * n, planes[k], sizeof(float) * n);
    for (u64 i = 0; i < n; i++) {
        aov[7 * n + i] = m.d_color.rad[i].r;
        aov[8 * n + i] = m.d_color.rad[i].g;
        aov[9 * n + i] = m.d_color.rad[i].b;
    }
    memcpy(shown, m.h_color.c, sizeof(u32) * n);
    c->color_pixels(SET_COLOR_TAG);
    memcpy(clean, m.h_color.c, sizeof(u32) * n);
}

// ---- the key block of the loop (TD/WinMain.cpp:186-209); keys: R W S Q E T = 1 2 4 8 16 32
void ref_motion_tick(ref_scene* s, int keys) {
    Input* in = s->input;
    Camera* cam = s->cam;
    const float cam_speed = .005f;  // TD/WinMain.cpp:171
    if (keys & 1) {
        in->set_quat((T_fp)0.0, (T_fp)0.09950371902099893, (T_fp)0.0, (T_fp)0.9950371902099893);
        s->obj1->transform(in, ROTATE_TRI_PY);
    }
    if (keys & 2) {
        in->set_quat(cam->o_prop.n.x, cam->o_prop.n.y, cam->o_prop.n.z, cam_speed);
        s->obj1->transform(in, TRANSLATE_Z);
    }
    if (keys & 4) {
        in->set_quat(cam->o_prop.n.x, cam->o_prop.n.y, cam->o_prop.n.z, -cam_speed);
        s->obj1->transform(in, TRANSLATE_Z);
    }
    if (keys & 8) {
        in->set_quat(cam->o_prop.u.x, cam->o_prop.u.y, cam->o_prop.u.z, cam_speed);
        s->obj1->transform(in, TRANSLATE_X);
    }
    if (keys & 16) {
        in->set_quat(cam->o_prop.u.x, cam->o_prop.u.y, cam->o_prop.u.z, -cam_speed);
        s->obj1->transform(in, TRANSLATE_X);
    }
    if (keys & 32) {
        in->set_quat((T_fp)0.0, (T_fp)-0.09950371902099893, (T_fp)0.0, (T_fp)0.9950371902099893);
        s->obj1->transform(in, ROTATE_TRI_NY);
    }
}

// ---- Object::transform with any vector and selector
void ref_motion_transform(ref_scene* s, const float t[4], int select) {
    s->input->set_quat(t[0], t[1], t[2], t[3]);
    s->obj1->transform(s->input, (u8)select);
}

void ref_motion_state(const ref_scene* s, float host_rot[12], float dev_rot[12], float quat[4], float init_face[4],
                      float cur_face[4]) {
    const Quaternion* q = s->obj1->quat;
    put4(q->rot_m->x, host_rot); put4(q->rot_m->y, host_rot + 4); put4(q->rot_m->z, host_rot + 8);
    put4(q->d_rot_m->x, dev_rot); put4(q->d_rot_m->y, dev_rot + 4); put4(q->d_rot_m->z, dev_rot + 8);
    put4(q->vec, quat);
    put4(s->obj1->init_face, init_face);
    put4(s->obj1->cur_face, cur_face);
}

}  // extern "C"
