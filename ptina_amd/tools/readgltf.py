'''
glTF 2.0 (.gltf JSON with external or base64 buffers, .glb) -> what the reference's loader
returns (tools/readgltf.py:15-240):  vertices [3n,8] f64, mtlids [n], materials as
((basecolor, tex), (metallic, tex), (roughness, tex)) 3-tuples, images as [x,y,c] arrays.
Written against the glTF specification with json/struct only (the reference uses gltflib).
'''

import base64
import io
import json
import os
import struct

import numpy as np

from . import matrix as mx

_COMP = {5120: np.int8, 5121: np.uint8, 5122: np.int16, 5123: np.uint16, 5125: np.uint32, 5126: np.float32}
_WIDTH = {'SCALAR': 1, 'VEC2': 2, 'VEC3': 3, 'VEC4': 4, 'MAT2': 4, 'MAT3': 9, 'MAT4': 16}


def _quaternion(q):
    x, y, z, w = q
    r = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (w * y + x * z)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    return mx.affine(r, np.zeros(3))


def readgltf(path):
    with open(path, 'rb') as fh:
        blob = fh.read()
    glb_bin = None
    if blob[:4] == b'glTF':
        _, _, total = struct.unpack_from('<III', blob, 0)
        off = 12
        doc = None
        while off < total:
            clen, ctype = struct.unpack_from('<II', blob, off)
            chunk = blob[off + 8:off + 8 + clen]
            if ctype == 0x4E4F534A:
                doc = json.loads(chunk.decode('utf-8'))
            elif ctype == 0x004E4942:
                glb_bin = chunk
            off += 8 + clen
    else:
        doc = json.loads(blob.decode('utf-8'))
    base = os.path.dirname(os.path.abspath(path))

    def load_uri(uri):
        if uri.startswith('data:'):
            return base64.b64decode(uri[uri.index('base64,') + 7:])
        with open(uri if os.path.isabs(uri) else os.path.join(base, uri), 'rb') as fh:
            return fh.read()

    buffers = [glb_bin if 'uri' not in b else load_uri(b['uri']) for b in doc.get('buffers', [])]
    views = []
    for v in doc.get('bufferViews', []):
        o = v.get('byteOffset', 0)
        views.append((buffers[v['buffer']][o:o + v['byteLength']], v.get('byteStride', 0)))

    def accessor(i):
        a = doc['accessors'][i]
        data, stride = views[a['bufferView']]
        comp, width = np.dtype(_COMP[a['componentType']]), _WIDTH[a['type']]
        o, count = a.get('byteOffset', 0), a['count']
        item = comp.itemsize * width
        if stride and stride != item:
            rows = [np.frombuffer(data, comp, width, o + k * stride) for k in range(count)]
            arr = np.stack(rows)
        else:
            arr = np.frombuffer(data, comp, count * width, o).reshape(count, width)
        return arr[:, 0] if width == 1 else arr

    images = []
    for im in doc.get('images', []):
        raw = load_uri(im['uri']) if 'uri' in im else views[im['bufferView']][0]
        from PIL import Image
        images.append(np.swapaxes(np.array(Image.open(io.BytesIO(raw))), 0, 1))

    materials = []
    for m in doc.get('materials', []):
        pbr = m.get('pbrMetallicRoughness', {})
        if 'metallicRoughnessTexture' in pbr:
            raise AssertionError('metallicRoughness texture not supported')      # as the reference
        # the reference hands the glTF TEXTURE index on as the image id, without going through textures[i].source
        # (readgltf.py:121-122); exporters write texture i -> image i, so the two coincide on its assets.  Kept as it is.
        tex = pbr.get('baseColorTexture', {}).get('index', -1)
        materials.append(((pbr.get('baseColorFactor', [1.0, 1.0, 1.0, 1.0]), tex),
                          (pbr.get('metallicFactor', 1.0), -1), (pbr.get('roughnessFactor', 1.0), -1)))

    prims = []

    def visit(ni, world):
        node = doc['nodes'][ni]
        if 'matrix' in node:
            local = np.array(node['matrix'], float).reshape(4, 4).T
        else:
            local = np.eye(4)
            if 'scale' in node:
                local = mx.scale(node['scale']) @ local
            if 'rotation' in node:
                local = _quaternion(node['rotation']) @ local
            if 'translation' in node:
                local = mx.translate(node['translation']) @ local
        world = world @ local
        if 'mesh' in node:
            for pr in doc['meshes'][node['mesh']]['primitives']:
                if pr.get('mode', 4) != 4:
                    continue
                at = pr['attributes']
                pos = accessor(at['POSITION'])
                nrm = accessor(at['NORMAL']) if 'NORMAL' in at else None
                uv = accessor(at['TEXCOORD_0']) if 'TEXCOORD_0' in at else None
                idx = accessor(pr['indices']).astype(np.int64) if 'indices' in pr else np.arange(pos.shape[0])
                prims.append((pos, nrm, uv, world, idx, pr.get('material')))
        for ch in node.get('children', []):
            visit(ch, world)

    scene = doc['scenes'][doc.get('scene', 0)]
    for ni in scene['nodes']:
        visit(ni, np.eye(4))

    arrays, mtlids = [], []
    for pos, nrm, uv, world, idx, mtl in prims:
        assert nrm is not None, 'primitive without normals'
        p = pos.astype(np.float64)[idx]
        n = nrm.astype(np.float64)[idx]
        t = np.zeros((p.shape[0], 2)) if uv is None else uv.astype(np.float64)[idx]
        ph = np.concatenate([p, np.ones((p.shape[0], 1))], axis=1) @ world.T
        p = ph[:, :3] / ph[:, 3:4]
        n = n @ world[:3, :3].T
        n = n / np.linalg.norm(n, axis=1, keepdims=True)
        a = np.concatenate([p, n, t], axis=1)
        assert a.shape[0] % 3 == 0
        arrays.append(a)
        mtlids.append(np.full(a.shape[0] // 3, -1 if mtl is None else mtl))
    assert arrays, 'no triangle primitives'
    return np.concatenate(arrays), np.concatenate(mtlids), materials, images


# ---------------------------------------------------------------- animated scenes: the node tree, skins, morph targets and animations
MAX_JOINTS, MAX_TARGETS = 256, 64          # what ModelPool.add_skin / add_morph_targets take (csrc/mpt_types.h MPT_DEFORM_MAX_*)
_PATHS = ('translation', 'rotation', 'scale', 'weights')


def _document(path):
    '''(the JSON document, accessor(i) -> array) of a .gltf or .glb file; sparse accessors are refused'''
    with open(path, 'rb') as fh:
        blob = fh.read()
    glb_bin, doc = None, None
    if blob[:4] == b'glTF':
        _, _, total = struct.unpack_from('<III', blob, 0)
        off = 12
        while off < total:
            clen, ctype = struct.unpack_from('<II', blob, off)
            chunk = blob[off + 8:off + 8 + clen]
            if ctype == 0x4E4F534A:
                doc = json.loads(chunk.decode('utf-8'))
            elif ctype == 0x004E4942:
                glb_bin = chunk
            off += 8 + clen
    else:
        doc = json.loads(blob.decode('utf-8'))
    base = os.path.dirname(os.path.abspath(path))

    def load_uri(uri):
        if uri.startswith('data:'):
            return base64.b64decode(uri[uri.index('base64,') + 7:])
        with open(uri if os.path.isabs(uri) else os.path.join(base, uri), 'rb') as fh:
            return fh.read()
    buffers = [glb_bin if 'uri' not in b else load_uri(b['uri']) for b in doc.get('buffers', [])]

    def accessor(i):
        a = doc['accessors'][i]
        if 'sparse' in a:
            raise NotImplementedError('%s: sparse accessors (accessor %d)' % (os.path.basename(path), i))
        v = doc['bufferViews'][a['bufferView']]
        o = v.get('byteOffset', 0)
        data, stride = buffers[v['buffer']][o:o + v['byteLength']], v.get('byteStride', 0)
        comp, width = np.dtype(_COMP[a['componentType']]), _WIDTH[a['type']]
        o, count = a.get('byteOffset', 0), a['count']
        if stride and stride != comp.itemsize * width:
            arr = np.stack([np.frombuffer(data, comp, width, o + k * stride) for k in range(count)])
        else:
            arr = np.frombuffer(data, comp, count * width, o).reshape(count, width)
        if a.get('normalized') and comp.kind in 'ui':
            arr = arr.astype(np.float32) / np.float32(np.iinfo(comp).max)
        return arr[:, 0] if width == 1 else arr
    return doc, accessor


def read_gltf_scene(path):
    '''a plain description of an animated glTF 2.0 file, nothing flattened: a dict of
      nodes       [dict(name, parent (-1: a root), children, translation [3], rotation [4] xyzw, scale [3], matrix [4,4] or None,
                  local [4,4] f64 = T R S or the matrix, mesh, skin (-1: none))]
      meshes      [dict(name, weights [T], primitives [dict(p, n [k,3,3], t [k,3,2] f32 in object space, material (-1: none), joints
                  [k,3,4] ints and weights [k,3,4] f32 or None, dp, dn [T,k,3,3] f32 or None)])]: triangles, expanded per face corner
      skins       [dict(joints [nj] node ids, inverse_bind [nj,4,4] f64, parents [nj] within the joint set (-1: a root), root_parent: the
                  node above the root joints (-1: none))], the joints ordered parents first
      animations  [dict(name, channels [dict(node, path 'translation' | 'rotation' | 'scale' | 'weights', interpolation, times, values)])],
                  times and values as tools.anim.track takes them
      roots       the scene's nodes;  joint_of {node: (skin, joint)};  carriers: the nodes that lead to a mesh, joints left out.
    NotImplementedError names what the file holds and this does not load: sparse accessors, required extensions, cameras, a second set
    of influences, a skin whose root joints have different parents or with a node that is no joint between two joints, a channel on a
    node that leads to no mesh, more joints or targets than ModelPool takes'''
    doc, accessor = _document(path)
    name = os.path.basename(path)
    if doc.get('extensionsRequired'):
        raise NotImplementedError('%s: required extensions (%s)' % (name, ', '.join(doc['extensionsRequired'])))
    if doc.get('cameras') or any('camera' in n for n in doc.get('nodes', [])):
        raise NotImplementedError('%s: cameras' % name)
    nodes = []
    for i, n in enumerate(doc.get('nodes', [])):
        t, r, s = (np.array(n.get(k, d), np.float64) for k, d in (('translation', [0, 0, 0]), ('rotation', [0, 0, 0, 1]), ('scale', [1, 1, 1])))
        matrix = np.array(n['matrix'], np.float64).reshape(4, 4).T.copy() if 'matrix' in n else None
        x, y, z, w = r
        R = np.array([[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - z * w), 2.0 * (x * z + y * w)],
                      [2.0 * (x * y + z * w), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - x * w)],
                      [2.0 * (x * z - y * w), 2.0 * (y * z + x * w), 1.0 - 2.0 * (x * x + y * y)]])
        local = np.eye(4)
        local[:3, :3], local[:3, 3] = R * s[None, :], t
        nodes.append(dict(name=n.get('name', 'node%d' % i), parent=-1, children=list(n.get('children', [])), translation=t, rotation=r, scale=s,
                          matrix=matrix, local=local if matrix is None else matrix, mesh=n.get('mesh', -1), skin=n.get('skin', -1)))
    for i, n in enumerate(nodes):
        for ch in n['children']:
            nodes[ch]['parent'] = i
    meshes = []
    for mi, m in enumerate(doc.get('meshes', [])):
        prims = []
        for pr in m['primitives']:
            if pr.get('mode', 4) != 4:
                continue
            at = pr['attributes']
            if 'JOINTS_1' in at or 'WEIGHTS_1' in at:
                raise NotImplementedError('%s: a second set of influences (JOINTS_1) on mesh %d' % (name, mi))
            pos = accessor(at['POSITION'])
            idx = accessor(pr['indices']).astype(np.int64) if 'indices' in pr else np.arange(pos.shape[0])
            k = idx.size // 3
            corner = lambda a, c, dt=np.float32: np.ascontiguousarray(np.asarray(a)[idx].reshape(k, 3, c), dt)      # noqa: E731
            p = corner(pos, 3)
            n_ = corner(accessor(at['NORMAL']), 3) if 'NORMAL' in at else np.zeros((k, 3, 3), np.float32)
            t_ = corner(accessor(at['TEXCOORD_0']), 2) if 'TEXCOORD_0' in at else np.zeros((k, 3, 2), np.float32)
            jt = corner(accessor(at['JOINTS_0']), 4, np.int64) if 'JOINTS_0' in at else None
            wt = corner(accessor(at['WEIGHTS_0']), 4) if 'WEIGHTS_0' in at else None
            targets = pr.get('targets', [])
            if len(targets) > MAX_TARGETS:
                raise NotImplementedError('%s: %d morph targets on mesh %d, more than the %d add_morph_targets takes' % (name, len(targets), mi, MAX_TARGETS))
            dp = np.stack([corner(accessor(tg['POSITION']), 3) if 'POSITION' in tg else np.zeros((k, 3, 3), np.float32) for tg in targets]) if targets else None
            dn = np.stack([corner(accessor(tg['NORMAL']), 3) if 'NORMAL' in tg else np.zeros((k, 3, 3), np.float32) for tg in targets]) if targets else None
            prims.append(dict(p=p, n=n_, t=t_, material=pr.get('material', -1), joints=jt, weights=wt, dp=dp, dn=dn))
        ntargets = prims[0]['dp'].shape[0] if prims and prims[0]['dp'] is not None else 0
        meshes.append(dict(name=m.get('name', 'mesh%d' % mi), weights=np.array(m.get('weights', [0.0] * ntargets), np.float64), primitives=prims))
    used = {n['skin'] for n in nodes if n['skin'] >= 0 and n['mesh'] >= 0}
    skins, joint_of = [], {}
    for si, sk in enumerate(doc.get('skins', [])):
        joints = list(sk['joints'])
        if len(joints) > MAX_JOINTS:
            raise NotImplementedError('%s: %d joints in skin %d, more than the %d add_skin takes' % (name, len(joints), si, MAX_JOINTS))
        ib = accessor(sk['inverseBindMatrices']).astype(np.float64).reshape(-1, 4, 4).transpose(0, 2, 1).copy() if 'inverseBindMatrices' in sk \
            else np.tile(np.eye(4), (len(joints), 1, 1))
        inside = set(joints)
        for j in joints:                                                   # the nearest joint above each joint; nothing but joints in between
            a, between = nodes[j]['parent'], False
            while a >= 0 and a not in inside:
                a, between = nodes[a]['parent'], True
            if a >= 0 and between:
                raise NotImplementedError('%s: a node that is no joint between two joints of skin %d (above node %d)' % (name, si, j))
        roots = [j for j in joints if nodes[j]['parent'] not in inside]
        if len({nodes[j]['parent'] for j in roots}) > 1:
            raise NotImplementedError('%s: skin %d has root joints with different parents' % (name, si))
        order, seen = [], set()                                            # parents first, as add_skeleton wants them; the file's indices are remapped
        def visit(j):      # noqa: E306
            if j in seen:
                return
            if nodes[j]['parent'] in inside:
                visit(nodes[j]['parent'])
            seen.add(j)
            order.append(j)
        for j in joints:
            visit(j)
        remap = [order.index(j) for j in joints]                            # the file's joint k is joint remap[k] here
        skins.append(dict(joints=order, inverse_bind=np.stack([ib[joints.index(j)] for j in order]), remap=np.array(remap, np.int64),
                          parents=np.array([order.index(nodes[j]['parent']) if nodes[j]['parent'] in inside else -1 for j in order], np.int64),
                          root_parent=nodes[roots[0]]['parent'] if roots else -1))
        if si in used:
            for k, j in enumerate(order):
                joint_of.setdefault(j, (si, k))
    for n in nodes:                                                         # a skinned primitive names joints in the file's order
        if n['skin'] >= 0 and n['mesh'] >= 0:
            for pr in meshes[n['mesh']]['primitives']:
                if pr['joints'] is not None and not pr.get('remapped'):
                    pr['joints'], pr['remapped'] = skins[n['skin']]['remap'][pr['joints']], True
    carriers = set()
    for i, n in enumerate(nodes):
        if n['mesh'] < 0:
            continue
        a = skins[n['skin']]['root_parent'] if n['skin'] >= 0 else i        # (a skinned node's own transform and ancestors play no part)
        while a >= 0:
            carriers.add(a)
            a = nodes[a]['parent']
    carriers -= set(joint_of)
    animations = []
    for ai, an in enumerate(doc.get('animations', [])):
        channels = []
        for ch in an['channels']:
            node, path = ch['target'].get('node', -1), ch['target']['path']
            sm = an['samplers'][ch['sampler']]
            interp = sm.get('interpolation', 'LINEAR')
            times, values = accessor(sm['input']).astype(np.float32), np.asarray(accessor(sm['output']), np.float32)
            ok = node in joint_of or (node in carriers and path != 'weights') or (path == 'weights' and node >= 0 and nodes[node]['mesh'] >= 0)
            if not ok:
                raise NotImplementedError('%s: a %s channel on node %d, which leads to no mesh' % (name, path, node))
            C = {'translation': 3, 'rotation': 4, 'scale': 3}.get(path) or (values.size // (times.size * (3 if interp == 'CUBICSPLINE' else 1)))
            values = values.reshape((times.size, 3, C) if interp == 'CUBICSPLINE' else (times.size, C))
            channels.append(dict(node=node, path=path, interpolation=interp, times=times, values=values))
        animations.append(dict(name=an.get('name', 'animation%d' % ai), channels=channels))
    return dict(nodes=nodes, meshes=meshes, skins=skins, animations=animations, roots=list(doc['scenes'][doc.get('scene', 0)]['nodes']),
                joint_of=joint_of, carriers=sorted(carriers))
