"""Writers for the Mitsuba 2.1.0 files the loader tests read (the reference ships no sample; these are synthetic
inputs written at test time): a hand-written scene that uses every element scene/mitsuba/*.rs knows, and a generated
SceneData (yuki_amd/scenes.py) as scene.xml + one binary PLY per mesh."""
import copy
import os

import numpy as np

import scene_files as sf


def _g(x):
    return "%.9g" % float(x)  # nine significant digits: a float32 survives the text round trip exactly


def _gs(v):
    return " ".join(_g(c) for c in v)


# ----------------------------------------------------------------------------- the hand-written scene
HAND_XML = """<?xml version="1.0" encoding="utf-8"?>
<!-- synthetic test scene: every element the reference's Mitsuba loader implements -->
<scene version="2.1.0">
  <default name="spp" value="64"/>
  <default name="resx" value="96"/>
  <default value='64' name='resy'/>
  <integrator type="path">
    <integer name="max_depth" value="8"/>
    <emitter type="point"><point name="nonsense"/></emitter>
  </integrator>
  <sensor type="perspective">
    <string name="fov_axis" value="%(fov_axis)s"/>
    <float name="fov" value="42.5"/>
    <float name="near_clip" value="0.01"/>
    <float name="far_clip" value="1e3"/>
    <transform name="to_world">
      <rotate x="1" angle="14.5"/>
      <rotate y="1" x="1e-3" angle="-8"/>
      <matrix value="0.995004165 0 0.0998334166 0 0 1 0 0 -0.0998334166 0 0.995004165 0 0 0 0 1"/>
      <translate value="0.75 2.25 -6.5"/>
    </transform>
    <sampler type="independent">
      <integer name="sample_count" value="$spp"/>
    </sampler>
    <film type="hdrfilm">
      <integer name="width" value="$resx"/>
      <integer name="height" value="$resy"/>
      <rfilter type="gaussian"><float name="stddev" value=".5"/></rfilter>
    </film>
  </sensor>

  <bsdf type="diffuse" id="grey">
    <rgb name="reflectance" value="0.6 0.55 0.5"/>
  </bsdf>
  <bsdf type="diffuse" id="half"/>
  <bsdf type="twosided" id="two_nested">
    <bsdf type="diffuse">
      <rgb name="reflectance" value="0.2 .7 3e-1"/>
    </bsdf>
  </bsdf>
  <bsdf type="twosided" id="two_direct">
    <rgb name="reflectance" value="0.8 0.3"/>
  </bsdf>
  <bsdf type="twosided" id="two_bare"/>
  <bsdf type="dielectric" id="glass">
    <float name="int_ior" value="1.33"/>
    <float name="ext_ior" value="1.0003"/>
    <rgb name="specular_reflectance" value="0.9 0.95 1"/>
    <rgb name="specular_transmittance" value=".95 1. 1e0"/>
  </bsdf>
  <bsdf type="dielectric" id="bk7"/>

  <emitter type="constant">
    <rgb name="radiance" value="9 9 9"/>
  </emitter>
  <emitter type="constant">
    <rgb name="radiance" value="0.15 0.2 0.3"/>
  </emitter>
  <emitter type="point">
    <point name="position" x="-2.5" z="-1.5" y="4"/>
    <rgb name="intensity" value="60 55 50"/>
  </emitter>
  <emitter type="area">
    <rgb name="radiance" value="1 1 1"/>
    <shape type="rectangle"><transform name="to_world"><scale value="1 2"/></transform></shape>
  </emitter>
  <emitter type="spot">
    <float name="cutoff_angle" value="35"/>
    <float name="beam_width" value="25"/>
    <transform name="to_world">
      <rotate x="1" angle="75"/>
      <rotate y="0.2" z="1" angle="20"/>
      <translate value="1.5 5 -1"/>
    </transform>
    <rgb name="intensity" value="150 160 170"/>
  </emitter>

  <shape type="ply">
    <string name="filename" value="cube.ply"/>
    <transform name="to_world">
      <translate value="-0.5 -1 -0.25"/>
      <scale value="12 0.5 8"/>
    </transform>
    <ref name="bsdf" id="grey"/>
  </shape>
  <bsdf type="diffuse" id="grey">
    <rgb name="reflectance" value="0.1 0.1 0.9"/>
  </bsdf>
  <shape type="ply">
    <ref id="glass" name="bsdf"/>
    <transform name="to_world">
      <scale value="4"/>
      <rotate x="0.3" y="1" z="-0.2" angle="33"/>
      <translate value="-1.5 0.5 0.25"/>
    </transform>
    <string name="filename" value="geo/cube_le.ply"/>
  </shape>
  <shape type="ply">
    <string name="filename" value="geo\\cube_be.ply"/>
    <transform name="to_world">
      <matrix value="2 0 0 1.25 0 1.5 0.5 0 0 -0.5 2 0.5 0 0 0 1"/>
    </transform>
    <ref name="bsdf" id="two_nested"/>
  </shape>
  <shape type="ply">
    <string name="filename" value="geo/cube_n.ply"/>
    <transform name="to_world">
      <scale value="3 3 3"/>
      <rotate z="1" angle="-25"/>
      <translate value="-3.5 0 -2"/>
    </transform>
    <ref name="bsdf" id="grey"/>
  </shape>
  <shape type="ply">
    <string name="filename" value="cube.ply"/>
    <transform name="to_world">
      <scale value="0.75"/>
      <translate value="2.75 0 -2.5"/>
    </transform>
    <ref name="bsdf" id="two_direct"/>
  </shape>
</scene>
"""


def write_hand_plys(dirname):
    """cube.ply (ASCII), geo/cube_le.ply (binary LE: normals, uvs, properties to skip), geo/cube_be.ply (binary BE, bare),
    geo/cube_n.ply (binary LE, normals only)."""
    os.makedirs(os.path.join(dirname, "geo"), exist_ok=True)
    sf.write_ascii_ply(os.path.join(dirname, "cube.ply"))
    sf.write_binary_ply(os.path.join(dirname, "geo", "cube_le.ply"), "<", normals=True, uvs=True, extra=True)
    sf.write_binary_ply(os.path.join(dirname, "geo", "cube_be.ply"), ">", normals=False, uvs=False, extra=False)
    sf.write_binary_ply(os.path.join(dirname, "geo", "cube_n.ply"), "<", normals=True, uvs=False, extra=True)


def write_hand_scene(dirname, fov_axis="x", name="scene.xml", text=None):
    """The hand-written scene (or `text` in its place) beside its four PLY files; returns the .xml path."""
    write_hand_plys(dirname)
    p = os.path.join(dirname, name)
    with open(p, "w", encoding="utf-8") as f:
        f.write(HAND_XML % dict(fov_axis=fov_axis) if text is None else text)
    return p


# ----------------------------------------------------------------------------- a generated SceneData as a Mitsuba file
def sensor_matrix(cam):
    """The `to_world` matrix of a Mitsuba sensor (+X left, +Y up, +Z forward, in Mitsuba's mirrored space) for a camera
    given in this project's space: float64 look-at, rounded to float32 by the nine-digit text."""
    S = np.array([-1.0, 1.0, 1.0])
    pos = np.asarray(cam["position"], dtype=np.float64) * S
    d = np.asarray(cam["target"], dtype=np.float64) * S - pos
    d /= np.linalg.norm(d)
    up = np.asarray(cam["up"], dtype=np.float64) * S
    left = np.cross(up, d)
    left /= np.linalg.norm(left)
    up = np.cross(d, left)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = left, up, d, pos
    return m


def write_scene_as_mitsuba(sd, dirname, res=(1920, 1080), extra_lights=(), twosided=False, name="scene.xml", reuse_meshes=False, reverse_winding=False):
    """A generated SceneData as scene.xml + meshes/m%05d.ply, what scene::mitsuba::load reads.  The loader mirrors
    everything by scale(-1, 1, 1), so x (and nx) is negated on the way out and the scene comes back as generated.

    What Mitsuba's subset cannot say is mapped, not dropped: glass -> `dielectric` (int_ior = the record's eta, both
    colours), every other material kind -> `diffuse` with the record's colour (sigma, roughness, eta / k are lost), an
    area light's quad stays as geometry with its (black) material, `rect` lights are not written.  extra_lights: dicts
    in MITSUBA's space — dict(kind="point", position=(x, y, z), I=(r, g, b)) or dict(kind="spot", cutoff=, beam=,
    I=, transform="<rotate .../><translate .../>").  reuse_meshes: do not write the PLY files, name the ones
    scene_files.write_scene_as_pbrt wrote into the same directory (the scene then loads mirrored).

    reverse_winding: write every face as (i0, i2, i1).  The loader flags every mesh as swapping handedness, so Triangle::intersect
    flips the geometric normal (shapes/triangle.rs:187-194): with the generator's winding a mesh without shading normals comes
    back inside out — the arrays are the generator's, but its shadow rays start below the surface and delta lights leave it
    black — while with the reversed winding the flip restores the generator's normals (what a Mitsuba exporter's files do: the
    mirror reverses their winding).  The index array then comes back with columns 1 and 2 exchanged.

    Returns (path, the SceneData that was written, per-file statistics)."""
    from yuki_amd import abi

    os.makedirs(os.path.join(dirname, "meshes"), exist_ok=True)
    out = ['<?xml version="1.0" encoding="utf-8"?>', '<scene version="2.1.0">']
    out.append('  <default name="resx" value="%d"/>\n  <default name="resy" value="%d"/>' % tuple(res))
    out.append('  <integrator type="path"><integer name="max_depth" value="8"/></integrator>')
    cam = sd.camera
    m = sensor_matrix(cam)
    for k in range(3):  # the loader refuses a camera matrix whose columns are not of unit length in float32 (sensor.rs:84-86)
        c = m[:3, k].astype(np.float32)
        ln = np.sqrt(((np.float32(0) + c[0] * c[0]) + c[1] * c[1]) + c[2] * c[2])
        assert abs(float(ln) - 1.0) <= float(np.finfo(np.float32).eps), "camera matrix column does not round to unit length"
    out.append('  <sensor type="perspective">\n    <string name="fov_axis" value="%s"/>\n    <float name="fov" value="%s"/>' % ("x" if cam["fov_axis"] == abi.FOV_X else "y", _g(cam["fov_degrees"])))
    out.append('    <transform name="to_world"><matrix value="%s"/></transform>' % _gs(m.reshape(16)))
    out.append('    <sampler type="independent"/>\n    <film type="hdrfilm"><integer name="width" value="$resx"/><integer name="height" value="$resy"/></film>\n  </sensor>')
    out.append('  <emitter type="constant"><rgb name="radiance" value="%s"/></emitter>' % _gs(sd.background))
    lights = []
    for l in sd.lights:
        if l["kind"] == "point":
            p = np.asarray(l["l2w"], dtype=np.float32)[:3, 3]
            lights.append(dict(kind="point", position=(-float(p[0]), float(p[1]), float(p[2])), I=tuple(l["I"])))
    lights += list(extra_lights)
    for l in lights:
        if l["kind"] == "point":
            out.append('  <emitter type="point"><point name="position" x="%s" y="%s" z="%s"/><rgb name="intensity" value="%s"/></emitter>' % (*(_g(v) for v in l["position"]), _gs(l["I"])))
        else:
            out.append('  <emitter type="spot"><float name="cutoff_angle" value="%s"/><float name="beam_width" value="%s"/><transform name="to_world">%s</transform><rgb name="intensity" value="%s"/></emitter>'
                       % (_g(l["cutoff"]), _g(l["beam"]), l["transform"], _gs(l["I"])))
    tri_mesh = np.asarray(sd.tri_mesh)
    order = np.argsort(tri_mesh, kind="stable")
    bounds = np.searchsorted(tri_mesh[order], np.arange(len(sd.meshes) + 1))
    materials, n_files = [], 0
    for mi, (has_n, has_uv, _swaps) in enumerate(sd.meshes):
        tri_ids = order[bounds[mi] : bounds[mi + 1]]
        assert len(tri_ids), "every mesh has triangles"
        tris = sd.indices[tri_ids].astype(np.int64)
        lo, hi = int(tris.min()), int(tris.max()) + 1
        mat = sd.materials[int(sd.tri_material[tri_ids[0]])]
        assert np.all(sd.tri_material[tri_ids] == sd.tri_material[tri_ids[0]]), "one material per mesh"
        ident = "m%05d" % mi
        if mat["kind"] == abi.MAT_GLASS:
            materials.append(dict(kind=abi.MAT_GLASS, a=tuple(mat["a"]), b=tuple(mat["b"]), c=float(mat["c"]), remap=False))
            out.append('  <bsdf type="dielectric" id="%s"><float name="int_ior" value="%s"/><rgb name="specular_reflectance" value="%s"/><rgb name="specular_transmittance" value="%s"/></bsdf>'
                       % (ident, _g(mat["c"]), _gs(mat["a"]), _gs(mat["b"])))
        else:
            materials.append(dict(kind=abi.MAT_MATTE, a=tuple(mat["a"]), b=(0.0, 0.0, 0.0), c=0.0, remap=False))
            inner = '<rgb name="reflectance" value="%s"/>' % _gs(mat["a"])
            if twosided:
                out.append('  <bsdf type="twosided" id="%s"><bsdf type="diffuse">%s</bsdf></bsdf>' % (ident, inner))
            else:
                out.append('  <bsdf type="diffuse" id="%s">%s</bsdf>' % (ident, inner))
        fn = "meshes/m%05d.ply" % mi
        if not reuse_meshes:
            mirror3 = np.array([-1.0, 1.0, 1.0], dtype=np.float32)
            sf.write_mesh_ply(os.path.join(dirname, fn), sd.points[lo:hi] * mirror3, (tris - lo)[:, [0, 2, 1]] if reverse_winding else tris - lo, sd.normals[lo:hi] * mirror3 if has_n else None, sd.uvs[lo:hi] if has_uv else None)
            n_files += 1
        out.append('  <shape type="ply"><string name="filename" value="%s"/><ref name="bsdf" id="%s"/></shape>' % (fn, ident))
    out.append("</scene>")
    p = os.path.join(dirname, name)
    with open(p, "w", encoding="utf-8") as f:
        f.write("\n".join(out) + "\n")
    written = copy.copy(sd)
    written.materials = materials
    written.tri_material = tri_mesh.astype(np.int32)
    written.tri_area_light = np.full(len(tri_mesh), -1, dtype=np.int32)
    written.meshes = [(bool(a), bool(b), True) for a, b, _ in sd.meshes]
    written.lights = lights
    if reverse_winding:
        written.indices = np.ascontiguousarray(sd.indices[:, [0, 2, 1]])
    return p, written, dict(ply_files=n_files, shapes=len(sd.meshes), lights=len(lights))
