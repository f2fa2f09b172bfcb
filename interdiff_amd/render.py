"""Pictures of a clip: ``visualize_body_obj`` of the reference's render/mesh_viz.py on the HIP rasteriser of csrc/render.hip.

The reference renders with pyrender + EGL + trimesh + imageio; none of them exists where this package runs.  The scene is the one the reference's
source fixes (see ``visualize_body_obj``), the picture is this package's own: nothing is pinned to pyrender's pixels.

PALETTE (the package's own table, RGB 0..255):
    body   past  light_grey  (204, 204, 204)      future  yellow_pale (226, 215, 132)
    object past  grey        (110, 110, 110)      future  pink        (255, 182, 193)
    ground inner (189, 195, 199)   outer (238, 238, 238)   -- the two values of the reference's mesh_utils.py
    markers past black (0, 0, 0)   future marker (31, 119, 180)
    background 'white' (255, 255, 255), 'black' (0, 0, 0), 'grey' (128, 128, 128)
"""
import ctypes as C
import math
import os
import warnings
import numpy as np
import torch
from . import _lib, geometry

PALETTE = dict(light_grey=(204, 204, 204), yellow_pale=(226, 215, 132), grey=(110, 110, 110), pink=(255, 182, 193), ground_inner=(189, 195, 199),
               ground_outer=(238, 238, 238), black=(0, 0, 0), marker=(31, 119, 180), white=(255, 255, 255), bg_grey=(128, 128, 128))
BACKGROUNDS = dict(white='white', black='black', grey='bg_grey')
AMBIENT = 0.3
LIGHT_INTENSITY = 5.0 / 3.0              # use_raymond_lighting(5.): each of the three lights at 5 / 3
OUTER_GROUND_DROP = 1e-3                 # metres the outer ground box sits below the inner one (in the reference the two top faces are coplanar)
MARKER_RADIUS = 0.01
DEFAULT_WORKSPACE = 256 << 20


def raymond_lights():
    """unit vectors towards the three "raymond" lights of mesh_utils.py (_add_raymond_light: the lights shine along -z of their nodes)"""
    th = [0.0, math.pi / 3.0, math.pi / 2.0]
    ph = [math.pi / 3.0, 2.0 * math.pi / 3.0, math.pi / 2.0]
    out = []
    for t, p in zip(th, ph):
        v = (math.sin(t) * math.cos(p), math.sin(t) * math.sin(p), math.cos(t))
        n = math.sqrt(sum(x * x for x in v))
        out += [x / n for x in v]
    return out


def make_scene(off=(0.0, 0.0, 0.0), bg_color='white'):
    """The camera, lights and background the reference's MeshViewer fixes: yfov = pi / 3, pose = translate(0, 2, 2.5) . rotate_x(-30 deg), near 0.05."""
    sc = _lib.RenderScene()
    sc.off[:] = [float(x) for x in off]
    sc.cam_t[:] = [0.0, 2.0, 2.5]
    sc.cam_cos, sc.cam_sin = math.cos(math.pi / 6), math.sin(math.pi / 6)
    sc.znear, sc.focal = 0.05, 1.0 / math.tan(math.pi / 6)
    sc.light[:] = raymond_lights()
    sc.light_gain, sc.ambient = LIGHT_INTENSITY / math.pi, AMBIENT
    bg = PALETTE[BACKGROUNDS[bg_color]] if isinstance(bg_color, str) else bg_color
    sc.bg[:] = [c / 255.0 for c in bg[:3]]
    return sc


def ground_mesh(minx, maxx, minz, maxz):
    """mesh_utils.py get_checkerboard_plane after its rotate_x(90 deg): two boxes centred at ((maxx - minx) / 2, (maxz - minz) / 2) -- NOT at the body's
    centre: the reference's own arithmetic -- with extents x 1 and x 1.6 of the body's range, 2e-6 thick, top at y = 0 (outer: OUTER_GROUND_DROP lower).
    Flat normals: four vertices per side.  -> verts, normals, rgb [48,3] float32, faces [24,3] int32"""
    ex, ez, cx, cz = maxx - minx, maxz - minz, (maxx - minx) / 2, (maxz - minz) / 2
    V, Nn, Cc, Fc = [], [], [], []
    for scale, col, drop in ((1.0, PALETTE['ground_inner'], 0.0), (1.6, PALETTE['ground_outer'], OUTER_GROUND_DROP)):
        lo = np.array([cx - scale * ex / 2, -2e-6 - drop, cz - scale * ez / 2])
        hi = np.array([cx + scale * ex / 2, 0.0 - drop, cz + scale * ez / 2])
        for axis in range(3):
            for side in (0, 1):
                u, w = (axis + 1) % 3, (axis + 2) % 3
                base = len(V)
                for a, b in ((0, 0), (1, 0), (1, 1), (0, 1)):
                    p = np.zeros(3)
                    p[axis], p[u], p[w] = (hi if side else lo)[axis], (hi if a else lo)[u], (hi if b else lo)[w]
                    V.append(p)
                    n = np.zeros(3)
                    n[axis] = 1.0 if side else -1.0
                    Nn.append(n)
                    Cc.append(np.asarray(col) / 255.0)
                Fc += [[base, base + 1, base + 2], [base, base + 2, base + 3]]
    return np.asarray(V, np.float32), np.asarray(Nn, np.float32), np.asarray(Cc, np.float32), np.asarray(Fc, np.int32)


def icosphere():
    """the 12 vertices (unit) and 20 faces of an icosahedron, outward winding"""
    g = (1 + 5 ** 0.5) / 2
    v = np.array([[-1, g, 0], [1, g, 0], [-1, -g, 0], [1, -g, 0], [0, -1, g], [0, 1, g], [0, -1, -g], [0, 1, -g], [g, 0, -1], [g, 0, 1], [-g, 0, -1], [-g, 0, 1]], np.float64)
    f = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
                  [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]], np.int32)
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32), f


class Mesh:
    """One mesh of a render call, on the device.  verts / normals [frames,V,3] (frames 1 or N), faces [F,3], rgb [N,3] per frame or [V,3] per vertex
    (``vertex_rgb``), optional per-frame pose R [N,3,3], t [N,3] applied inside the kernel, ``scene_space`` for a mesh that does not turn with the views."""

    def __init__(self, verts, normals, faces, rgb, R=None, t=None, scene_space=False, vertex_rgb=False, device='cuda'):
        f = lambda a, dt: None if a is None else torch.as_tensor(a).to(device=device, dtype=dt).contiguous()
        self.verts, self.normals, self.faces, self.rgb, self.R, self.t = f(verts, torch.float32), f(normals, torch.float32), f(faces, torch.int32), \
            f(rgb, torch.float32), f(R, torch.float32), f(t, torch.float32)
        if self.verts.dim() == 2:
            self.verts, self.normals = self.verts[None], self.normals[None]
        if self.verts.shape != self.normals.shape or self.verts.dim() != 3 or self.verts.shape[2] != 3 or self.faces.dim() != 2 or self.faces.shape[1] != 3:
            raise ValueError('mesh: verts / normals [frames,V,3] and faces [F,3] expected')
        self.flags = (_lib.RMESH_SCENE_SPACE if scene_space else 0) | (_lib.RMESH_VERTEX_RGB if vertex_rgb else 0)

    def check(self, N):
        V = self.verts.shape[1]
        if self.rgb.shape != ((V, 3) if self.flags & _lib.RMESH_VERTEX_RGB else (N, 3)):
            raise ValueError('mesh: rgb must be [V,3] with vertex_rgb, else [N,3]')
        if self.R is not None and (self.t is None or tuple(self.R.shape) != (N, 3, 3) or tuple(self.t.shape) != (N, 3)):
            raise ValueError('mesh: R [N,3,3] and t [N,3] come together')

    def struct(self):
        m = _lib.RenderMesh()
        m.verts, m.normals, m.faces, m.rgb = self.verts.data_ptr(), self.normals.data_ptr(), self.faces.data_ptr(), self.rgb.data_ptr()
        m.R, m.t = (self.R.data_ptr(), self.t.data_ptr()) if self.R is not None else (None, None)
        m.V, m.F, m.frames, m.flags = self.verts.shape[1], self.faces.shape[0], self.verts.shape[0], self.flags
        return m


def render_frames(scene, meshes, N, views, h, w, want_id=False, want_depth=False, want_setup=False, workspace_bytes=None, stage_ms=False):
    """interdiff_render_frames on device meshes -> dict(rgb uint8 [N,views,h,w,3], dropped, and id / depth / setup / stage_ms when asked for).
    ``workspace_bytes`` caps the workspace: the images are then rendered in chunks, with identical bits."""
    lib = _lib.load()
    for m in meshes:
        m.check(N)
    dev = meshes[0].verts.device
    arr = (_lib.RenderMesh * len(meshes))(*[m.struct() for m in meshes])
    Ft = sum(m.faces.shape[0] for m in meshes)
    one = lib.interdiff_render_frames_workspace_bytes(1, Ft, h, w)
    full = lib.interdiff_render_frames_workspace_bytes(N * views, Ft, h, w)
    if one == 0:
        raise ValueError('render_frames: h, w must be in 1..%d' % _lib.RENDER_MAX_DIM)
    nbytes = min(full, max(one, DEFAULT_WORKSPACE if workspace_bytes is None else int(workspace_bytes)))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    rgb = torch.empty(N, views, h, w, 3, dtype=torch.uint8, device=dev)
    ids = torch.empty(N, views, h, w, dtype=torch.int32, device=dev) if want_id else None
    depth = torch.empty(N, views, h, w, dtype=torch.int32, device=dev) if want_depth else None
    setup = torch.empty(N, views, 2 * Ft, _lib.RENDER_REC_INTS, dtype=torch.int32, device=dev) if want_setup else None
    dropped, ms = C.c_int64(0), (C.c_float * 3)()
    _lib.check(lib.interdiff_render_frames(C.byref(scene), arr, len(meshes), N, views, h, w, _lib.dptr(rgb), _lib.dptr(ids, allow_none=True),
                                           _lib.dptr(depth, allow_none=True), _lib.dptr(setup, allow_none=True), C.byref(dropped),
                                           ms if stage_ms else None, _lib.dptr(ws), nbytes, _lib.stream()), 'render_frames')
    out = dict(rgb=rgb, dropped=int(dropped.value))
    if want_id:
        out['id'] = ids
    if want_depth:
        out['depth'] = depth
    if want_setup:
        out['setup'] = setup
    if stage_ms:
        out['stage_ms'] = dict(setup=ms[0], bin=ms[1], tile_resolve=ms[2])
    return out


def _dev(x, device):
    if isinstance(x, torch.Tensor):
        return x.to(device=device)                       # a device tensor stays where it is
    return torch.from_numpy(np.ascontiguousarray(x)).to(device)


def _colours(T, past_len, past, future, device):
    i = torch.arange(T, device=device)
    c = torch.tensor([PALETTE[past], PALETTE[future]], dtype=torch.float32, device=device) / 255.0
    return c[(i > past_len).long()].contiguous()         # frames i <= past_len are "past"


def build_clip(body_verts, body_face, obj_verts, obj_face, past_len=0, pcd=None, bg_color='white', obj_R=None, obj_t=None, device='cuda'):
    """The scene of visualize_body_obj as (idf scene, [Mesh ...], T) -- see there."""
    bv = _dev(body_verts, device).float().contiguous()
    T = bv.shape[0]
    bf = _dev(body_face, device).to(torch.int32).contiguous()
    of = _dev(obj_face, device).to(torch.int32).contiguous()
    ov = _dev(obj_verts, device).float().contiguous()
    # the reference's centring, on the NEGATED body over the whole clip: x, z on the bounding box's centre, the floor at the minimum height
    lo, hi = (-bv).amin(dim=(0, 1)).tolist(), (-bv).amax(dim=(0, 1)).tolist()
    minx, maxx, minz, maxz = lo[0], hi[0], lo[2], hi[2]
    scene = make_scene(((minx + maxx) / 2, lo[1], (minz + maxz) / 2), bg_color)
    gv, gn, gc, gf = ground_mesh(minx, maxx, minz, maxz)
    meshes = [Mesh(gv, gn, gf, gc, scene_space=True, vertex_rgb=True, device=device)]
    if pcd is not None:
        # markers as instanced icospheres, in the body's coordinates; black for the past, one colour after (per-body-part colouring is out of scope)
        p = _dev(pcd, device).float().reshape(T, -1, 3)
        iv, ifc = icosphere()
        iv_d, M = torch.from_numpy(iv).to(device), p.shape[1]
        mv = (p[:, :, None, :] + MARKER_RADIUS * iv_d).reshape(T, M * 12, 3)
        mn = iv_d.repeat(M, 1)[None].expand(T, -1, -1)
        mf = (torch.from_numpy(ifc).to(device)[None] + 12 * torch.arange(M, device=device, dtype=torch.int32)[:, None, None]).reshape(-1, 3)
        meshes.append(Mesh(mv, mn, mf, _colours(T, past_len, 'black', 'marker', device), device=device))
    if obj_R is not None:
        on = geometry.vertex_normals(ov.reshape(1, -1, 3), of)
        meshes.append(Mesh(ov.reshape(1, -1, 3), on, of, _colours(T, past_len, 'grey', 'pink', device), R=_dev(obj_R, device).float().reshape(T, 3, 3),
                           t=_dev(obj_t, device).float().reshape(T, 3), device=device))
    else:
        meshes.append(Mesh(ov, geometry.vertex_normals(ov, of), of, _colours(T, past_len, 'grey', 'pink', device), device=device))
    meshes.append(Mesh(bv, geometry.vertex_normals(bv, bf), bf, _colours(T, past_len, 'light_grey', 'yellow_pale', device), device=device))
    return scene, meshes, T


def tile_views(rgb):
    """[T,4,h,w,3] -> [T,h,4w,3] in the reference's order: views 0, 1, 3, 2 side by side"""
    return torch.cat([rgb[:, 0], rgb[:, 1], rgb[:, 3], rgb[:, 2]], dim=2)


def frame_duration_ms(sample_rate=1):
    """GIF frame time for 30 // sample_rate frames per second, on the format's 10 ms grid"""
    return int(round(100.0 / (30 // sample_rate))) * 10


def save_video(video, save_path, sample_rate=1):
    """video uint8 [T,rows,cols,3] -> ``.gif`` (PIL, 30 // sample_rate fps) or, for any other path, a directory of PNG frames"""
    from PIL import Image
    frames = [Image.fromarray(f) for f in video]
    if str(save_path).lower().endswith('.gif'):
        frames[0].save(save_path, save_all=True, append_images=frames[1:], duration=frame_duration_ms(sample_rate), loop=0)
    else:
        os.makedirs(save_path, exist_ok=True)
        for i, f in enumerate(frames):
            f.save(os.path.join(save_path, '%05d.png' % i))


def visualize_body_obj(body_verts, body_face, obj_verts, obj_face, past_len=0, pcd=None, multi_angle=True, h=512, w=512, bg_color='white',
                       save_path=None, sample_rate=1, obj_R=None, obj_t=None, workspace_bytes=None):
    """render/mesh_viz.py visualize_body_obj: body_verts [T,Vb,3], body_face [Fb,3], obj_verts [T,Vo,3], obj_face [Fo,3] (numpy arrays or device
    tensors; device tensors are rendered where they are) -> uint8 [T,3,h,4w] (``multi_angle``: views 0, 1, 3, 2 side by side) or [T,3,h,w].
    With ``obj_R`` [T,3,3] and ``obj_t`` [T,3], obj_verts is ONE canonical mesh [Vo,3] posed per frame inside the kernel.

    The scene is the one the reference's source fixes: all coordinates negated; x and z centred on the body's bounding box over the whole clip, the floor
    at the body's minimum height; the ground two thin boxes with extents x 1 and x 1.6 of the body's range; body and object in their "past" colours for
    frames i <= past_len, "future" after; views 1-3 successive quarter turns of the meshes about y with ground and lights fixed; camera yfov = pi / 3 at
    translate(0, 2, 2.5) . rotate_x(-30 deg), near plane 0.05; the three "raymond" lights at intensity 5 / 3 each.
    Shading: Lambert on smooth vertex normals (the vertex_normals kernel) plus an ambient term (0.3), per vertex, min(1, .) -- interpolated in screen
    space.  The face winding is not reversed: nothing is culled and the normals are given, so it cannot be seen.

    DEPARTURES (pyrender cannot run here, so nothing is pinned to its pixels): no shadow maps; no metallic-roughness BRDF; ``MeshViewer.set_cam_trans``,
    which moves the camera every time a mesh is added, is not reproduced (its effect depends on pyrender internals); the outer ground box is lowered by
    1 mm (coplanar with the inner one in the reference, where the GL depth test decides pixel by pixel); markers (``pcd``) are placed in the body's
    coordinates and have one colour.  The palette is this module's own (head of the file).
    LIMIT: a triangle that is partly in view but has a snapped vertex further than 2048 pixels from the image's corner is left out and counted, never
    clamped; a ``RuntimeWarning`` reports the count (``render_frames`` returns it as ``dropped``).  In this scene that is the ground of a clip that
    walks far: its outer box reaches z = 1.3 x the body's z-range in front of the origin, meets the camera's near plane at z ~ 3.6 m (a z-range beyond
    ~2.7 m) and its clipped corners then project tens of thousands of pixels away at 512 x 512 -- those ground triangles vanish.  Render such clips
    in shorter windows (the ground is sized per call).
    ``save_path``: ``*.gif`` is written through PIL at 30 // sample_rate fps; any other path is a directory that receives PNG frames."""
    dev = body_verts.device if isinstance(body_verts, torch.Tensor) and body_verts.is_cuda else 'cuda'
    scene, meshes, T = build_clip(body_verts, body_face, obj_verts, obj_face, past_len, pcd, bg_color, obj_R, obj_t, dev)
    views = 4 if multi_angle else 1
    out = render_frames(scene, meshes, T, views, h, w, workspace_bytes=workspace_bytes)
    if out['dropped']:
        warnings.warn('visualize_body_obj: %d triangles were left out of the %d images: they are partly in view but reach beyond the guard band of '
                      '+-%d pixels (see the docstring: typically the ground of a clip that walks several metres)' % (
                          out['dropped'], T * views, _lib.RENDER_GUARD // _lib.RENDER_SUBPIX), RuntimeWarning, stacklevel=2)
    rgb = out['rgb']
    video = (tile_views(rgb) if multi_angle else rgb[:, 0]).cpu().numpy()
    if save_path is not None:
        save_video(video, save_path, sample_rate)
    return np.ascontiguousarray(np.transpose(video, (0, 3, 1, 2)))
