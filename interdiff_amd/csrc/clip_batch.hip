// A training batch from a device-resident clip set in a fixed number of launches (interdiff_amd/dataset.py DeviceClipSet.assemble).
//
// clip_canon_kernel        data/dataset_smpl.py:105-152, 171-179 for B clips at once: one workgroup per clip, one lane per frame.  Gathers the T
//                          frames at stride sample_rate, canonicalises them (csrc/clip_canon.h, double, rounded once), writes the raw [T,B,.] fields,
//                          the frame's column of gt [B,1,144,T] (model/diffusion_smpl.py:212-214), the foot-ground labels and the clip's object cloud.
//                          Every lane derives the first frame's origin and heading itself (a handful of double operations) -- no LDS, no barrier.
// clip_body_records_kernel data/dataset_smpl.py:134-139, 167-169, 189: human_verts [T,B,V,7] = vertex | normal | contact label, markers [T,B,67,7] and
//                          contact_label [T,B,V] of one frame per workgroup.  The frame's contact list (CSR) is expanded into an LDS byte map (plain
//                          stores of 1: a vertex named twice stores 1 twice, no atomics); the [V,7] record is then written as ONE flat run of floats,
//                          16 bytes per lane where the run is 16-byte aligned (a frame is 28 V bytes, so every other frame starts 8 bytes off: the
//                          few floats before the first and after the last aligned quad go out as single stores).  Without vertices it writes the
//                          labels alone.
#include "common.h"
#include "clip_canon.h"

namespace {

// global frame of (clip b, clip frame t), or -1 when the clip does not lie inside its sequence (the host checks before it launches; this keeps
// a bad table from ever becoming an address)
__device__ __forceinline__ int64_t clip_frame(const idf_clip_set &cs, const int32_t *__restrict__ clips, int B, int T, int rate, int b, int t, int *local) {
    const int sid = clips[b], start = clips[B + b];
    if (sid < 0 || sid >= cs.n_seq || start < 0) return -1;
    const int64_t first = cs.seq_off[sid], len = cs.seq_off[sid + 1] - first;
    if ((int64_t)start + (int64_t)(T - 1) * rate >= len) return -1;
    *local = start + t * rate;
    return first + *local;
}

__global__ __launch_bounds__(128) void clip_canon_kernel(idf_clip_set cs, const int32_t *__restrict__ clips, int B, int T, int rate, idf_clip_batch out) {
    const int b = blockIdx.x, t = threadIdx.x;
    int l0 = 0, lt = 0;
    const int64_t g0 = clip_frame(cs, clips, B, T, rate, b, 0, &l0);
    if (g0 < 0) return;
    const int sid = clips[b];
    // the clip's object cloud: [P,6] as stored and its positions [P,3]
    const float *src = cs.obj_points6 + (size_t)sid * cs.P * 6;
    for (int i = t; i < cs.P * 6; i += blockDim.x) {
        const float v = src[i];
        out.obj_points6[(size_t)b * cs.P * 6 + i] = v;
        const int p = i / 6, c = i - 6 * p;
        if (c < 3) out.obj_points[((size_t)b * cs.P + p) * 3 + c] = v;
    }
    if (t >= T) return;
    const int64_t g = clip_frame(cs, clips, B, T, rate, b, t, &lt);
    clipc::Frame0 f0;
    clipc::frame0_of(cs.fit64 + g0 * 12, cs.joints + g0 * 9, f0);
    const size_t tb = (size_t)t * B + b;
    const float *pose = cs.pose + g * 156;
    float root[3];
    clipc::canon_frame(f0, cs.fit64 + g * 12, cs.joints + g * 9, pose, root, out.body_trans + tb * 3, out.obj_angles + tb * 3, out.obj_trans + tb * 3,
                       out.pelvis + tb * 3, out.gt + (size_t)b * 144 * T + t, T);
    float *bp = out.body_pose + tb * 66, *hp = out.hand_pose + tb * 90, *be = out.beta + tb * 10;
    for (int k = 0; k < 3; ++k) bp[k] = root[k];
    for (int k = 3; k < 66; ++k) bp[k] = pose[k];
    for (int k = 0; k < 90; ++k) hp[k] = pose[66 + k];
    for (int k = 0; k < 10; ++k) be[k] = cs.betas[g * 10 + k];
    float gl = 0.f, gr = 0.f;
    if (lt > 0) {
        gl = clipc::foot_still(cs.joints + g * 9 + 3, cs.joints + (g - 1) * 9 + 3);
        gr = clipc::foot_still(cs.joints + g * 9 + 6, cs.joints + (g - 1) * 9 + 6);
    } else {
        const int lab = cs.first_label[sid];          // 10: left, 11: right (checked on the host)
        gl = lab == 10 ? 1.f : 0.f;
        gr = lab == 11 ? 1.f : 0.f;
    }
    out.ground[tb * 2] = gl;
    out.ground[tb * 2 + 1] = gr;
    if (t == 0) {
        for (int k = 0; k < 3; ++k) out.centroid[b * 3 + k] = (float)f0.centroid[k];
        for (int k = 0; k < 9; ++k) out.rotation[b * 9 + k] = (float)f0.R[k];
    }
}

constexpr int REC_THREADS = 256;

__device__ __forceinline__ float record_elem(const float *__restrict__ v, const float *__restrict__ nr, const unsigned char *lab, int64_t e) {
    const int vtx = (int)(e / 7), c = (int)(e - 7 * (int64_t)vtx);
    return c < 3 ? v[3 * vtx + c] : (c < 6 ? nr[3 * vtx + c - 3] : (float)lab[vtx]);
}

template <bool BODY>
__global__ __launch_bounds__(REC_THREADS) void clip_body_records_kernel(idf_clip_set cs, const int32_t *__restrict__ clips, int B, int T, int rate,
                                                                        const float *__restrict__ verts, const float *__restrict__ normals,
                                                                        const int32_t *__restrict__ frame_map, float *__restrict__ human_verts,
                                                                        float *__restrict__ markers, unsigned char *__restrict__ contact_label) {
    extern __shared__ unsigned char lab[];            // [V] contact byte map of this frame
    const int tid = threadIdx.x, V = cs.V;
    const int64_t n = frame_map ? frame_map[blockIdx.x] : (int64_t)blockIdx.x;      // destination frame t * B + b
    if (n < 0 || n >= (int64_t)T * B) return;
    const int t = (int)(n / B), b = (int)(n - (int64_t)t * B);
    int local = 0;
    const int64_t g = clip_frame(cs, clips, B, T, rate, b, t, &local);
    if (g < 0) return;
    for (int i = tid; i < V; i += REC_THREADS) lab[i] = 0;
    __syncthreads();
    for (int e = cs.body_ptr[g] + tid; e < cs.body_ptr[g + 1]; e += REC_THREADS) {
        const int v = cs.body_idx[e];
        if ((unsigned)v < (unsigned)V) lab[v] = 1;
    }
    __syncthreads();
    if (contact_label)
        for (int i = tid; i < V; i += REC_THREADS) contact_label[(size_t)n * V + i] = lab[i];
    if (!BODY) return;
    const float *v = verts + (size_t)blockIdx.x * V * 3, *nr = normals + (size_t)blockIdx.x * V * 3;
    const int64_t s = n * V * 7, e_end = s + (int64_t)V * 7;      // this frame's run in the flat output (the base pointer is 16-byte aligned)
    const int64_t a = (s + 3) & ~(int64_t)3, z = e_end & ~(int64_t)3;
    for (int64_t q = a / 4 + tid; q < z / 4; q += REC_THREADS) {
        const int64_t e = 4 * q - s;
        const float4 o = make_float4(record_elem(v, nr, lab, e), record_elem(v, nr, lab, e + 1), record_elem(v, nr, lab, e + 2), record_elem(v, nr, lab, e + 3));
        reinterpret_cast<float4 *>(human_verts)[q] = o;
    }
    if (tid < a - s && s + tid < e_end) human_verts[s + tid] =record_elem(v, nr, lab, tid);                       // < 4 floats in front of the first aligned quad
    if (z >= a && tid < e_end - z) human_verts[z + tid] = record_elem(v, nr, lab, z - s + tid);      // < 4 floats behind the last one
    for (int i = tid; i < cs.n_markers * 7; i += REC_THREADS) {
        const int m = i / 7, c = i - 7 * m, vtx = cs.markers_idx[m];
        if ((unsigned)vtx < (unsigned)V) markers[(size_t)n * cs.n_markers * 7 + i] = record_elem(v, nr, lab, (int64_t)vtx * 7 + c);
    }
}

bool set_ok(const idf_clip_set *cs) {
    return cs && cs->n_seq > 0 && cs->P > 0 && cs->V > 0 && cs->n_markers >= 0 && cs->seq_off && cs->pose && cs->betas && cs->fit64 && cs->joints && cs->obj_points6 &&
           cs->first_label && cs->body_ptr && cs->body_idx && (cs->n_markers == 0 || cs->markers_idx);
}

constexpr int CLIP_MAX_T = 128, CLIP_MAX_V = 65536;      // one lane per frame; the byte map must fit the default 64 KiB of LDS

}  // namespace

extern "C" int interdiff_clip_batch(const idf_clip_set *cs, const int32_t *clips, int32_t B, int32_t T, int32_t sample_rate, const idf_clip_batch *out, void *stream) {
    if (!set_ok(cs) || !clips || !out || B <= 0 || T <= 0 || T > CLIP_MAX_T || sample_rate <= 0 || cs->V > CLIP_MAX_V) return IDF_E_INVAL;
    if (!out->body_pose || !out->hand_pose || !out->body_trans || !out->obj_angles || !out->obj_trans || !out->pelvis || !out->beta || !out->gt || !out->ground ||
        !out->centroid || !out->rotation || !out->obj_points || !out->obj_points6)
        return IDF_E_INVAL;
    hipStream_t s = idf_stream(stream);
    hipLaunchKernelGGL(clip_canon_kernel, dim3((unsigned)B), dim3(T <= 64 ? 64 : 128), 0, s, *cs, clips, B, T, sample_rate, *out);
    if (out->contact_label)
        hipLaunchKernelGGL(clip_body_records_kernel<false>, dim3((unsigned)((int64_t)T * B)), dim3(REC_THREADS), (size_t)cs->V, s, *cs, clips, B, T, sample_rate,
                           (const float *)nullptr, (const float *)nullptr, (const int32_t *)nullptr, (float *)nullptr, (float *)nullptr, out->contact_label);
    IDF_CHECK_LAUNCH();
    return IDF_OK;
}

extern "C" int interdiff_clip_body_records(const idf_clip_set *cs, const int32_t *clips, int32_t B, int32_t T, int32_t sample_rate, const float *verts,
                                           const float *normals, const int32_t *frame_map, int64_t n_frames, float *human_verts, float *markers,
                                           uint8_t *contact_label, void *stream) {
    if (!set_ok(cs) || !clips || B <= 0 || T <= 0 || T > CLIP_MAX_T || sample_rate <= 0 || cs->V > CLIP_MAX_V || !verts || !normals || !human_verts || !markers ||
        n_frames < 0 || n_frames > (int64_t)T * B || ((uintptr_t)human_verts & 15))
        return IDF_E_INVAL;
    if (n_frames == 0) return IDF_OK;
    hipLaunchKernelGGL(clip_body_records_kernel<true>, dim3((unsigned)n_frames), dim3(REC_THREADS), (size_t)cs->V, idf_stream(stream), *cs, clips, B, T, sample_rate,
                       verts, normals, frame_map, human_verts, markers, contact_label);
    IDF_CHECK_LAUNCH();
    return IDF_OK;
}

// HOST instance of the per-clip math: the T frames of ONE clip, already gathered.  fit double [T,12], pelvis fp32 [T,3], pose fp32 [T,156];
// rotation_override fp32 [9] or null (then the heading of frame 0 decides, as in the kernel).
extern "C" int interdiff_debug_clip_canon(const double *fit, const float *pelvis, const float *pose, int32_t T, const float *rotation_override, float *root,
                                          float *trans, float *obj_angle, float *obj_trans, float *pelvis_out, float *gt, float *centroid, float *rotation) {
    if (!fit || !pelvis || !pose || T <= 0 || !root || !trans || !obj_angle || !obj_trans || !pelvis_out || !gt || !centroid || !rotation) return IDF_E_INVAL;
    clipc::Frame0 f0;
    if (rotation_override) clipc::frame0_with_rotation(rotation_override, pelvis, f0);
    else clipc::frame0_of(fit, pelvis, f0);
    for (int t = 0; t < T; ++t)
        clipc::canon_frame(f0, fit + 12 * t, pelvis + 3 * t, pose + 156 * t, root + 3 * t, trans + 3 * t, obj_angle + 3 * t, obj_trans + 3 * t, pelvis_out + 3 * t,
                           gt + t, T);
    for (int k = 0; k < 3; ++k) centroid[k] = (float)f0.centroid[k];
    for (int k = 0; k < 9; ++k) rotation[k] = (float)f0.R[k];
    return IDF_OK;
}
