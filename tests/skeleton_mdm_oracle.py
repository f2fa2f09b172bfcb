"""CPU restatement of the HO-GCN skeleton denoiser (model/diffusion_skeleton.py ``MDM``), built from the layer functions of
oracle/denoiser.py: the decoder / encoder stacks are the SMPL model's at feed-forward width ``ff_size``; what differs is the
shape embedding on the encoder side (:204-210) and the head (:218-248): ``objFinalLinear`` gives 7 pose values and the 36
object-keypoint channels of x0 are ``calc_obj_pred(pose, zero_pose_obj)``.  Any dtype (the tests run it in fp64 and fp32)."""
import torch
from oracle import denoiser as oden

N_BODY, N_POINTS = 63, 12


def quaternion_to_matrix(q):
    """pytorch3d.transforms.quaternion_to_matrix on (w, x, y, z): NOT normalised, two_s = 2 / (q . q)."""
    r, i, j, k = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    s2 = 2.0 / (q * q).sum(-1)
    rows = [1 - s2 * (j * j + k * k), s2 * (i * j - k * r), s2 * (i * k + j * r),
            s2 * (i * j + k * r), 1 - s2 * (i * i + k * k), s2 * (j * k - i * r),
            s2 * (i * k - j * r), s2 * (j * k + i * r), 1 - s2 * (i * i + j * j)]
    return torch.stack(rows, dim=-1).reshape(q.shape[:-1] + (3, 3))


def calc_obj_pred(pose, zero_pose_obj):
    """:218-229.  pose [T,B,7] (translation | quaternion xyzw), zero_pose_obj [B,P,3] -> [T,B,P,3]."""
    quat = torch.cat([pose[:, :, -1, None], pose[:, :, -4:-1]], dim=2)
    R = quaternion_to_matrix(quat)[:, :, None]                                   # [T,B,1,3,3]
    return (R @ zero_pose_obj[None, :, :, :, None] + pose[:, :, None, :3, None])[..., 0]


def _pe(sd, like):
    pe = sd['PositionalEmbedding.pe'][:, 0] if 'PositionalEmbedding.pe' in sd else oden.positional_table()
    return pe.to(like.dtype)


def forward(sd, x, ts, zero_pose_obj, cond, n_body=N_BODY, n_points=N_POINTS):
    """:231-257.  x [B,1,106,T], ts int64 [B], zero_pose_obj [B,12,3], cond [M,B,256] -> x0 [B,1,106,T]."""
    pe = _pe(sd, x)
    xt = x.squeeze(1).permute(2, 0, 1)                                           # [T,B,C]
    T, B, _ = xt.shape
    h = (oden._lin(xt[..., :n_body], sd, 'bodyEmbedding') + oden._lin(xt[..., n_body:n_body + 3 * n_points], sd, 'objEmbedding')
         + oden.time_embedding(sd, ts, pe))
    h = h + pe[:T, None]
    for l in range(oden.N_LAYERS):
        p = 'decoder.layers.%d' % l
        h = oden.qan_layer(h, cond, sd, p) if l in oden.QAN_LAYERS else oden.std_layer(h, cond, sd, p)
    body, pose = oden._lin(h, sd, 'bodyFinalLinear'), oden._lin(h, sd, 'objFinalLinear')
    obj = calc_obj_pred(pose, zero_pose_obj).reshape(T, B, -1)
    return torch.cat([body, obj, pose], dim=2).permute(1, 2, 0).unsqueeze(1).contiguous()


def get_embeddings(sd, body_gt, obj_gt, pose_gt, zero_pose_obj, past_len=10):
    """:194-215.  body_gt [T,B,21,3], obj_gt [T,B,12,3], pose_gt [T,B,7], zero_pose_obj [B,12,3] -> (cond [past,B,256], gt [T,B,106])."""
    T, B = body_gt.shape[:2]
    body, obj = body_gt.reshape(T, B, -1), obj_gt.reshape(T, B, -1)
    gt = torch.cat([body, obj, pose_gt], dim=2)
    h = (oden._lin(body[:past_len], sd, 'bodyEmbedding') + oden._lin(obj[:past_len], sd, 'objEmbedding')
         + oden._lin(zero_pose_obj.reshape(1, B, -1), sd, 'shapeEmbedding'))
    h = h + _pe(sd, h)[:past_len, None]
    for l in range(oden.N_LAYERS):
        p = 'encoder.layers.%d' % l
        h = oden.enc_qan_layer(h, sd, p) if l in oden.QAN_LAYERS else oden.enc_std_layer(h, sd, p)
    return h, gt
