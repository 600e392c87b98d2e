"""Predictions to pixels: ``MeshRenderer`` draws the predicted hand mesh and the posed object over the crop the network saw, and the
depth / face maps later work needs (silhouettes, visible surfaces, occlusion).  The device side is ``ops.MeshRaster`` (csrc/raster.hip:
vpho_mesh_raster_f32, vpho_render_overlay_u8; the rules are in include/vpho_hip.h); it stands in for the reference's pytorch3d renderer
(lib/utils/render_fn.py, lib/dataset/base.py:472-500,632-688) and is NOT compared with it: pytorch3d's rasteriser has its own coverage and
blending rules, the ones here are this project's own, chosen to be exact and watertight.  ``write_png`` / ``read_png`` need ``zlib`` and
``struct`` only.  Imported only when asked for (``--infer_render N``)."""
import struct
import zlib

import numpy as np
import torch

from . import ops
from . import physics_eval
from .frames import IMG_MEAN, IMG_STD

HAND_COLOUR, OBJ_COLOUR = (224.0, 160.0, 128.0), (96.0, 160.0, 224.0)
N_HAND_VERTS = 778


class MeshRenderer:
    """One raster table holding the hand mesh (``assets['mano']['faces']``, 778 vertices; mesh 0) and every object of
    ``physics_eval.object_meshes(assets)`` (meshes 1 ..), with the objects' rest vertices on the device."""

    def __init__(self, assets, device, asset_root='asset'):
        self.device = torch.device(device)
        hand_faces = np.asarray(assets['mano']['faces'])
        objs = physics_eval.object_meshes(assets, asset_root)
        self.obj_names = list(objs.keys())
        self.obj_index = {n: i for i, n in enumerate(self.obj_names)}
        self.raster = ops.MeshRaster([(N_HAND_VERTS, hand_faces)] + [(len(objs[n]['verts']), objs[n]['faces']) for n in self.obj_names], self.device)
        self.obj_vmax = max(len(objs[n]['verts']) for n in self.obj_names)
        rest = np.zeros((len(self.obj_names), self.obj_vmax, 3), np.float32)
        for i, n in enumerate(self.obj_names):
            rest[i, :len(objs[n]['verts'])] = objs[n]['verts']
        self.obj_rest = torch.from_numpy(rest).to(self.device)
        self.hand_colour, self.obj_colour, self.opacity, self.ambient = HAND_COLOUR, OBJ_COLOUR, 0.75, 0.3

    def obj_ids(self, names):
        """object names -> positions among the objects (host list): a KeyError names an object the assets lack"""
        try:
            return [self.obj_index[n] for n in names]
        except KeyError as e:
            raise KeyError(f'MeshRenderer: object {e.args[0]!r} is not in the asset table') from None

    @staticmethod
    def _size(size):
        return (int(size), int(size)) if np.isscalar(size) else (int(size[0]), int(size[1]))

    def depth_maps(self, verts, mesh_id, K, size, z_near=0.01, back=True):
        """verts (n,Vmax,3) camera-frame metres, mesh_id n ids into the table (0 = hand, 1 + k = object k), K (n,3,3), size = side or
        (H, W) -> the dict of ``ops.MeshRaster.raster``: depth_front / depth_back in METRES (0 where empty), face_front / face_back (-1)."""
        H, W = self._size(size)
        return self.raster.raster(verts, mesh_id, K, H, W, z_near=z_near, back=back)

    def pose_objects(self, obj_ids, obj_rt, mirror=None):
        """rest vertices of the named objects under [R | t] (n,3,4): R v + t, fp32 -> (n, obj_vmax, 3); ``mirror`` (n,) bool negates x
        afterwards (the frame of a mirrored left-hand crop).  Rows beyond an object's vertex count are padding no face names."""
        idx = torch.as_tensor(obj_ids, dtype=torch.long, device=self.device)
        rt = obj_rt.to(self.device).float()
        r = self.obj_rest[idx]
        # element-wise, in a fixed order: an image's vertices do not depend on what else is in the batch
        v = ((r[..., 0:1] * rt[:, None, :, 0] + r[..., 1:2] * rt[:, None, :, 1]) + r[..., 2:3] * rt[:, None, :, 2]) + rt[:, None, :, 3]
        if mirror is not None:
            sign = torch.where(mirror.to(self.device).bool(), -1.0, 1.0).to(v.dtype)
            v = torch.cat([v[..., :1] * sign[:, None, None], v[..., 1:]], -1)
        return v.contiguous()

    def object_depth_maps(self, obj_names, obj_rt, K, size, background_val=0.0, z_near=0.01):
        """The contract of the reference's ``get_obj_front_and_back_depth_map`` (lib/dataset/base.py:632-688) for a batch: the objects'
        full meshes under ``obj_rt`` (n,3,4) seen through ``K`` (n,3,3) -> depth_front, depth_back (n,H,W) fp32 in MILLIMETRES with
        ``background_val`` where nothing covers the pixel, front_face_map, back_face_map (n,H,W) int32 with -1 there.  The back map is the
        FARTHEST covering face; the reference takes the farthest of its 20 nearest layers (faces_per_pixel), which is the same surface for
        any object of fewer than 20 layers along a ray.  The reference's cache stores the depths as whole millimetres; these are not
        truncated."""
        ids = self.obj_ids(obj_names)
        maps = self.depth_maps(self.pose_objects(ids, obj_rt), [1 + i for i in ids], K, size, z_near=z_near)
        empty = maps['face_front'] < 0
        front = torch.where(empty, torch.full_like(maps['depth_front'], background_val), maps['depth_front'] * 1000.0)
        back = torch.where(empty, torch.full_like(maps['depth_back'], background_val), maps['depth_back'] * 1000.0)
        return front, back, maps['face_front'], maps['face_back']

    def overlay(self, batch, out, result=None):
        """The predicted hand and object over ``batch['rgb']`` (n,3,P,P), in the frame of the crop the network saw -> (n,P,P,3) uint8.
        Camera ``batch['cam_intr_crop_flip']``; hand ``out['agg_hand_vert'] + batch['root_joint_flip']`` (the mirrored frame the network
        predicts in); object: the full mesh of ``batch['obj_name']`` under ``ops.obj_9d_to_rt(out['agg_obj_6d'], batch['root_joint'])`` with x
        negated for left hands -- what the aggregation projects into the crop (csrc/aggregate.hip obj_heat_kernel: R v + t + root_joint,
        then the flip), so a left hand's object lands where the mirrored image shows it.  Two raster launches and one overlay launch on
        the current stream, no wait."""
        rgb = batch['rgb']
        n, _, H, W = rgb.shape
        K = batch['cam_intr_crop_flip'].double()
        hand_v = (out['agg_hand_vert'].float() + batch['root_joint_flip'].float()[:, None]).contiguous()
        hand = self.raster.raster(hand_v, [0] * n, K, H, W, back=False)
        ids = self.obj_ids(batch['obj_name'])
        rt = ops.obj_9d_to_rt(out['agg_obj_6d'].double().contiguous(), batch['root_joint'].float().contiguous())
        obj_v = self.pose_objects(ids, rt, mirror=~batch['is_right'].bool())
        obj = self.raster.raster(obj_v, [1 + i for i in ids], K, H, W, back=False)
        return self.raster.overlay(rgb, K, hand=dict(hand, colour=self.hand_colour, opacity=self.opacity),
                                   obj=dict(obj, colour=self.obj_colour, opacity=self.opacity), mean=IMG_MEAN, std=IMG_STD, ambient=self.ambient,
                                   out=result)


# ---------------------------------------------------------------------------------------------------------------------- PNG
_PNG_MAGIC = b'\x89PNG\r\n\x1a\n'


def _chunk(kind, data):
    return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', zlib.crc32(kind + data) & 0xFFFFFFFF)


def png_bytes(rgb_u8, level=6):
    """(H,W,3) uint8 -> the bytes of an 8-bit RGB PNG: IHDR, one IDAT (every scanline with filter type 0), IEND"""
    a = np.ascontiguousarray(rgb_u8)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f'write_png: an image of shape {a.shape} / {a.dtype}, expected (H, W, 3) uint8')
    H, W, _ = a.shape
    raw = np.concatenate([np.zeros((H, 1), np.uint8), a.reshape(H, W * 3)], 1).tobytes()
    return _PNG_MAGIC + _chunk(b'IHDR', struct.pack('>IIBBBBB', W, H, 8, 2, 0, 0, 0)) + _chunk(b'IDAT', zlib.compress(raw, level)) + _chunk(b'IEND', b'')


def write_png(path, rgb_u8):
    with open(path, 'wb') as f:
        f.write(png_bytes(rgb_u8))
    return path


def read_png(path):
    """the inverse of ``write_png`` for 8-bit RGB files without interlace (filter types 0-4 are undone, every CRC is checked)"""
    with open(path, 'rb') as f:
        data = f.read()
    if data[:8] != _PNG_MAGIC:
        raise ValueError(f'read_png: {path} is not a PNG file')
    pos, idat, shape = 8, [], None
    while pos < len(data):
        length, kind = struct.unpack('>I', data[pos:pos + 4])[0], data[pos + 4:pos + 8]
        body = data[pos + 8:pos + 8 + length]
        if struct.unpack('>I', data[pos + 8 + length:pos + 12 + length])[0] != (zlib.crc32(kind + body) & 0xFFFFFFFF):
            raise ValueError(f'read_png: {path}: chunk {kind!r} fails its CRC')
        if kind == b'IHDR':
            W, H, depth, colour, comp, filt, lace = struct.unpack('>IIBBBBB', body)
            if (depth, colour, comp, filt, lace) != (8, 2, 0, 0, 0):
                raise ValueError(f'read_png: {path}: only 8-bit RGB without interlace is read')
            shape = (H, W)
        elif kind == b'IDAT':
            idat.append(body)
        elif kind == b'IEND':
            break
        pos += 12 + length
    if shape is None:
        raise ValueError(f'read_png: {path} has no IHDR chunk')
    H, W = shape
    rows = np.frombuffer(zlib.decompress(b''.join(idat)), np.uint8).reshape(H, 1 + 3 * W)
    out = np.zeros((H, 3 * W), np.uint8)
    for y in range(H):
        ft, line = int(rows[y, 0]), rows[y, 1:].astype(np.int32)
        prev = out[y - 1].astype(np.int32) if y else np.zeros(3 * W, np.int32)
        if ft == 0:
            cur = line
        elif ft == 2:
            cur = (line + prev) & 255
        elif ft in (1, 3, 4):
            cur = np.zeros(3 * W, np.int32)
            for i in range(3 * W):
                left = cur[i - 3] if i >= 3 else 0
                if ft == 1:
                    pred = left
                elif ft == 3:
                    pred = (left + prev[i]) // 2
                else:
                    ul = prev[i - 3] if i >= 3 else 0
                    p = left + prev[i] - ul
                    pa, pb, pc = abs(p - left), abs(p - prev[i]), abs(p - ul)
                    pred = left if pa <= pb and pa <= pc else prev[i] if pb <= pc else ul
                cur[i] = (line[i] + pred) & 255
        else:
            raise ValueError(f'read_png: {path}: filter type {ft}')
        out[y] = cur.astype(np.uint8)
    return out.reshape(H, W, 3)
