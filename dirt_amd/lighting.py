"""`dirt.lighting` over torch tensors (dirt/lighting.py:1-344): mesh normals and simple reflectance models.

Same signatures and conventions as the reference: `vertices` [*, V, 3|4] with any leading batch dimensions and a
topology `faces` [F, 3] shared by the batch.  Where the reference builds a sparse [F, V, ...] tensor and reduces
it (dirt/lighting.py:64-79) this uses one `index_add_` over the vertex axis -- same sums, linear memory."""
import ctypes
import math
import numbers

import torch


def _prepare_vertices_and_faces(vertices, faces):
    if not isinstance(vertices, torch.Tensor):
        vertices = torch.as_tensor(vertices, dtype=torch.float32)
    faces = torch.as_tensor(faces, device=vertices.device)
    assert faces.dtype in (torch.int32, torch.int64)  # dirt/lighting.py:15-17
    return vertices, faces.long()


def _get_face_normals(vertices, faces):
    # vertices [*, V, 3], faces [F, 3] -> unit normals [*, F, 3] (dirt/lighting.py:21-28)
    v0, v1, v2 = (vertices[..., faces[:, k], :] for k in range(3))
    n = torch.linalg.cross(v1 - v0, v2 - v0, dim=-1)
    return n / (torch.linalg.vector_norm(n, dim=-1, keepdim=True) + 1.e-12)


def vertex_normals(vertices, faces, name=None):
    """Per-vertex normals: the normalised sum of the unit normals of the faces using the vertex
    (dirt/lighting.py:31-89).  [*, V, 3|4] -> [*, V, 3]."""
    vertices, faces = _prepare_vertices_and_faces(vertices, faces)
    vertices = vertices[..., :3]
    assert vertices.dim() in (2, 3)  # as the reference (dirt/lighting.py:59)
    normals_by_face = _get_face_normals(vertices, faces)  # [*, F, 3]
    summed = torch.zeros_like(vertices)
    for k in range(3):
        summed = summed.index_add(-2, faces[:, k], normals_by_face)
    return summed / (torch.linalg.vector_norm(summed, dim=-1, keepdim=True) + 1.e-12)


def vertex_normals_pre_split(vertices, faces, name=None, static=False):
    """`vertex_normals` for meshes where every vertex belongs to exactly one face (dirt/lighting.py:97-129):
    each vertex gets its face's unit normal (not renormalised; vertices used by no face get zero)."""
    vertices, faces = _prepare_vertices_and_faces(vertices, faces)
    vertices = vertices[..., :3]
    normals_by_face = _get_face_normals(vertices, faces)  # [*, F, 3]
    out = torch.zeros_like(vertices)
    for k in range(3):
        out = out.index_add(-2, faces[:, k], normals_by_face)  # scatter_nd sums duplicates, as tf.scatter_nd does
    return out


def split_vertices_by_face(vertices, faces, name=None):
    """An equivalent mesh in which each vertex is used by exactly one face (dirt/lighting.py:132-172):
    returns (new_vertices [*, 3F, 3|4], new_faces [F, 3] = arange(3F))."""
    vertices, faces = _prepare_vertices_and_faces(vertices, faces)
    new_vertices = vertices[..., faces.reshape(-1), :]
    new_faces = torch.arange(faces.shape[0] * 3, dtype=torch.int32, device=vertices.device).reshape(-1, 3)
    return new_vertices, new_faces


def _as(x, like):
    return x if isinstance(x, torch.Tensor) else torch.as_tensor(x, dtype=like.dtype, device=like.device)


def _clamp_cosines(cosines, double_sided):
    return torch.abs(cosines) if double_sided else torch.clamp(cosines, min=0.)


def diffuse_directional(vertex_normals, vertex_colors, light_direction, light_color, double_sided=True, name=None):
    """Lambertian reflectance under one directional light (dirt/lighting.py:175-218).  Normals and the light
    direction are assumed normalised.  [*, V, 3], [*, V, C], [*, 3], [*, C] -> [*, V, C]."""
    vertex_normals = _as(vertex_normals, torch.zeros((), dtype=torch.float32))
    vertex_colors = _as(vertex_colors, vertex_normals)
    light_direction = _as(light_direction, vertex_normals)
    light_color = _as(light_color, vertex_normals)
    cosines = torch.matmul(vertex_normals, -light_direction[..., None])  # [*, V, 1]
    cosines = _clamp_cosines(cosines, double_sided)
    return light_color[..., None, :] * vertex_colors * cosines


def specular_directional(vertex_positions, vertex_normals, vertex_reflectivities, light_direction, light_color,
                         camera_position, shininess, double_sided=True, name=None):
    """Phong reflectance under one directional light (dirt/lighting.py:221-283), including the reference's
    placement of the 1e-12 (added to the normalised view vector, dirt/lighting.py:274)."""
    vertex_positions = _as(vertex_positions, torch.zeros((), dtype=torch.float32))
    vertex_normals = _as(vertex_normals, vertex_positions)
    vertex_reflectivities = _as(vertex_reflectivities, vertex_positions)
    light_direction = _as(light_direction, vertex_positions)
    light_color = _as(light_color, vertex_positions)
    camera_position = _as(camera_position, vertex_positions)
    shininess = _as(shininess, vertex_positions)
    to_light = -light_direction
    reflected = -to_light[..., None, :] + 2. * torch.matmul(vertex_normals, to_light[..., None]) * vertex_normals
    to_camera = camera_position[..., None, :] - vertex_positions
    cosines = torch.sum((to_camera / torch.linalg.vector_norm(to_camera, dim=-1, keepdim=True) + 1.e-12) * reflected,
                        dim=-1, keepdim=True)
    cosines = _clamp_cosines(cosines, double_sided)
    return light_color[..., None, :] * vertex_reflectivities * torch.pow(cosines, shininess[..., None, None])


def diffuse_point(vertex_positions, vertex_normals, vertex_colors, light_position, light_color, double_sided=True,
                  name=None):
    """Lambertian reflectance under one point light (dirt/lighting.py:286-344).  As in the reference the cosine
    is taken between the normal and the direction FROM the light TO the point."""
    vertex_positions = _as(vertex_positions, torch.zeros((), dtype=torch.float32))
    vertex_normals = _as(vertex_normals, vertex_positions)
    vertex_colors = _as(vertex_colors, vertex_positions)
    light_position = _as(light_position, vertex_positions)
    light_color = _as(light_color, vertex_positions)
    relative = vertex_positions - light_position[..., None, :]
    incident = relative / (torch.linalg.vector_norm(relative, dim=-1, keepdim=True) + 1.e-12)
    cosines = _clamp_cosines(torch.sum(vertex_normals * incident, dim=-1), double_sided)
    return light_color[..., None, :] * vertex_colors * cosines[..., None]


# ---- second-order spherical-harmonic irradiance.  Not in the reference: the light model of differentiable face and body
# fitting, 9 coefficients per colour channel.  This is the specification `shading.shade_gbuffer_sh` implements per pixel
# (DESIGN.md §7b).

SH_C0, SH_C1, SH_C2 = 0.28209479177387814, 0.4886025119029199, 1.0925484305920792
SH_C3, SH_C4 = 0.31539156525252005, 0.5462742152960396
SH_BAND = (0, 1, 1, 1, 2, 2, 2, 2, 2)   # the band l of basis function k
SH_LAMBERT = (3.141592653589793, 2.0943951023931953, 0.7853981633974483)   # band_scale: radiance coefficients -> Lambertian irradiance


def sh_basis(normals):
    """The nine real spherical harmonics of bands 0-2 at `normals` [..., 3] (taken as given, not normalised) -> [..., 9],
    in the order (l, m) = (0,0), (1,-1), (1,0), (1,1), (2,-2), (2,-1), (2,0), (2,1), (2,2); orthonormal over the unit sphere."""
    normals = _as(normals, torch.zeros((), dtype=torch.float32))
    x, y, z = normals[..., 0], normals[..., 1], normals[..., 2]
    return torch.stack([SH_C0 * torch.ones_like(x), SH_C1 * y, SH_C1 * z, SH_C1 * x,
                        SH_C2 * (x * y), SH_C2 * (y * z), SH_C3 * (3. * (z * z) - 1.), SH_C2 * (x * z), SH_C4 * (x * x - y * y)], dim=-1)


def spherical_harmonics(vertex_normals, vertex_colors, coefficients, band_scale=(1., 1., 1.), normalize=False):
    """Reflectance under spherical-harmonic lighting: colour_j * sum_k band_scale[band(k)] * coefficients[k, j] * Y_k(normal).
    [*, V, 3], [*, V, 3], coefficients [K, 3] -- or [B, K, 3] against normals whose first axis is B -- with K in (1, 4, 9)
    (whole bands; the missing ones are zero) -> [*, V, 3].  band_scale: three numbers, one per band (SH_LAMBERT turns
    radiance coefficients into irradiance).  normalize: the normals go through torch.nn.functional.normalize
    (n / max(|n|, 1e-12)) first; otherwise they are taken as given, as everywhere in this module."""
    vertex_normals = _as(vertex_normals, torch.zeros((), dtype=torch.float32))
    vertex_colors = _as(vertex_colors, vertex_normals)
    coefficients = _as(coefficients, vertex_normals)
    if coefficients.dim() not in (2, 3) or coefficients.shape[-1] != 3 or coefficients.shape[-2] not in (1, 4, 9):
        raise ValueError('coefficients must have shape [K, 3] or [B, K, 3] with K in (1, 4, 9), got %s' % list(coefficients.shape))
    scale = [float(s) for s in band_scale]
    if len(scale) != 3:
        raise ValueError('band_scale must be 3 numbers, got %d' % len(scale))
    if normalize:
        vertex_normals = torch.nn.functional.normalize(vertex_normals, dim=-1, eps=1.e-12)
    K = coefficients.shape[-2]
    weights = torch.tensor([scale[b] for b in SH_BAND[:K]], dtype=vertex_normals.dtype, device=vertex_normals.device)
    basis = sh_basis(vertex_normals)[..., :K] * weights   # [*, V, K]
    if coefficients.dim() == 3:   # one table per leading batch entry: [B, 1.., K, 3]
        coefficients = coefficients.reshape((coefficients.shape[0],) + (1,) * (basis.dim() - 2) + (K, 3))
    irradiance = (basis[..., None] * coefficients).sum(-2)
    return vertex_colors * irradiance


# ---- Cook-Torrance metallic-roughness reflectance (GGX distribution, Smith-Schlick visibility, Schlick Fresnel).  Not in the
# reference: the material model of inverse rendering.  This is the specification `shading.shade_gbuffer_pbr` implements per
# pixel.

PBR_KINDS = ('directional', 'point')


def cook_torrance_lobes(vertex_positions, vertex_normals, vertex_colors, roughness, metalness, camera_position, lights,
                        min_roughness=0.04, dielectric_f0=0.04):
    """The two lobes of `cook_torrance` apart: a list, per light, of (diffuse, specular, weight, products) with diffuse =
    kd c / pi and specular = D Vis F ([*, V, 3] each), weight = light colour * max(n^ . l, 0) and products = n^ * l, the three
    products n^ . l adds up; the light's term is (diffuse + specular) * weight."""
    min_roughness, dielectric_f0 = float(min_roughness), float(dielectric_f0)
    if not 0. < min_roughness <= 1.:
        raise ValueError('min_roughness must be > 0 and <= 1, got %r' % min_roughness)
    if not 0. <= dielectric_f0 <= 1.:
        raise ValueError('dielectric_f0 must lie in [0, 1], got %r' % dielectric_f0)
    p = _as(vertex_positions, torch.zeros((), dtype=torch.float32))
    n, c, r, mu, cam = (_as(x, p) for x in (vertex_normals, vertex_colors, roughness, metalness, camera_position))
    normalize = lambda x: torch.nn.functional.normalize(x, dim=-1, eps=1.e-12)   # noqa: E731
    dot = lambda a, b: torch.sum(a * b, dim=-1, keepdim=True)   # noqa: E731
    nh_ = normalize(n)
    v = normalize(cam[..., None, :] - p)
    r, mu = r[..., None], mu[..., None]
    rho = torch.clamp(r, min_roughness, 1.)
    a2 = (rho * rho) * (rho * rho)
    k = (rho + 1.) * (rho + 1.) / 8.
    f0 = dielectric_f0 * (1. - mu) + c * mu
    nv = torch.clamp(dot(nh_, v), min=0.)
    lobes = []
    for i, rec in enumerate(lights):
        if not isinstance(rec, (tuple, list)) or len(rec) != 3 or rec[0] not in PBR_KINDS:
            raise ValueError('light %d: expected (%s, vector, color), got %r' % (i, ' or '.join(repr(s) for s in PBR_KINDS), rec))
        d, kc = _as(rec[1], p), _as(rec[2], p)
        l = normalize(-d[..., None, :]).expand_as(p) if rec[0] == 'directional' else normalize(d[..., None, :] - p)
        h = normalize(l + v)
        nl, nh, vh = (torch.clamp(dot(a, b), min=0.) for a, b in ((nh_, l), (nh_, h), (v, h)))
        x = torch.linalg.cross(nh_, h, dim=-1)
        den = dot(x, x) + torch.mul(a2, nh * nh)   # a call, not an operator: tests/shade_pbr_reference.py cuts the autograd path here
        D = a2 / (torch.pi * (den * den))
        vis = 0.25 / ((nl * (1. - k) + k) * (nv * (1. - k) + k))
        w = 1. - vh
        F = f0 + (1. - f0) * (((w * w) * (w * w)) * w)
        kd = (1. - F) * (1. - mu)
        lobes.append((kd * c / torch.pi, (D * vis) * F, kc[..., None, :] * nl, nh_ * l))
    return lobes


def cook_torrance(vertex_positions, vertex_normals, vertex_colors, roughness, metalness, camera_position, lights,
                  min_roughness=0.04, dielectric_f0=0.04, visibility=None):
    """Metallic-roughness reflectance under directional and point lights, summed.
    positions, normals, colours (albedo) [*, V, 3]; roughness, metalness [*, V]; camera_position [*, 3];
    lights: records ('directional', direction [*, 3], color [*, 3]) or ('point', position [*, 3], color [*, 3]) -> [*, V, 3]
    (zeros without lights).  Per point (every normalisation is torch.nn.functional.normalize, x / max(|x|, 1e-12)):

        n^ = normalize(n)                     v = normalize(cam - p)
        rho = clamp(r, min_roughness, 1)      a2 = (rho^2)^2                  k = (rho + 1)^2 / 8
        F0_j = dielectric_f0 (1 - mu) + c_j mu                                nv = max(n^ . v, 0)
        per light:  l = normalize(-d) (directional)  |  normalize(d - p) (point: towards the light; no distance fall-off)
                    h = normalize(l + v)      nl = max(n^ . l, 0)   nh = max(n^ . h, 0)   vh = max(v . h, 0)
                    D   = a2 / (pi den^2),  den = |n^ x h|^2 + a2 nh^2
                    Vis = 0.25 / ((nl (1 - k) + k) (nv (1 - k) + k))
                    w = 1 - vh,  F_j = F0_j + (1 - F0_j) ((w w)(w w) w)       kd_j = (1 - F_j)(1 - mu)
                    L_j = (kd_j c_j / pi + D Vis F_j) color_j nl          with visibility:  ... ((color_j nl) s)

    visibility: None or [*, V, L], one factor s per light (`shadow_visibility`'s output): a plain multiplication of the light's
    weight, not clamped; all ones give the bits of the call without it.
    `den` is written with the cross product (|n^ x h|^2 = 1 - nh^2 for unit vectors): the subtractive form nh^2 (a2 - 1) + 1
    loses four decimal digits in float32 at low roughness.  `Vis` is the Smith-Schlick term with the 4 nl nv of the
    microfacet denominator cancelled: nothing divides by a cosine.  min_roughness in (0, 1] and dielectric_f0 in [0, 1] are
    python numbers."""
    lobes = cook_torrance_lobes(vertex_positions, vertex_normals, vertex_colors, roughness, metalness, camera_position, lights,
                                min_roughness, dielectric_f0)
    p = _as(vertex_positions, torch.zeros((), dtype=torch.float32))
    total = torch.zeros_like(_as(vertex_colors, p) + p)
    if visibility is not None:
        visibility = _as(visibility, p)
        if visibility.shape[-1] != len(lobes):
            raise ValueError('visibility has %d channels for %d lights' % (visibility.shape[-1], len(lobes)))
    for i, (diffuse, specular, weight, _) in enumerate(lobes):
        if visibility is not None:
            weight = weight * visibility[..., i:i + 1]
        total = total + (diffuse + specular) * weight
    return total


# ---- split-sum image-based lighting.  Not in the reference: the material of `cook_torrance` under an environment.  The lobe's
# integral against the environment is split into the environment filtered by the lobe (`texture.prefilter_cube`) times the
# lobe's own integral against a white environment, which depends on (n . v, roughness) alone and is tabulated once by
# `environment_brdf`.  These are the specifications `shading.shade_gbuffer_ibl` implements per pixel.

def environment_brdf(size=32, samples=(512, 128)):
    """The split-sum scale and bias of `cook_torrance`'s specular lobe -> [size, size, 2] float32 (A, B): texel (i, j) holds
    nv = (j + 0.5) / size (columns) and rho = (i + 0.5) / size (rows), and with n = (0, 0, 1), v = (sqrt(1 - nv^2), 0, nv),
    a2, k, D, Vis as in `cook_torrance` and Fc = (1 - vh)^5

        A = integral of D Vis (1 - Fc) nl dl        B = integral of D Vis Fc nl dl        over the hemisphere of l,

    so that a constant environment of radiance 1 reflects F0 A + B.  Computed in float64 on the CPU by a fixed quadrature, a
    stratified GGX importance sampling of the half vector h: with u the distribution function of the density D nh,
    tan^2 theta_h = a2 u / (1 - u), and l = 2 vh h - v has the density D nh / (4 vh), which cancels D.  The strata are the
    samples[0] x samples[1] cells of equal size in (y, phi), y = log(u / (1 - u)) in [-40, 40] (du = u (1 - u) dy) and phi over
    the half circle (the integrand is even in phi), sampled at their midpoints: equal cells in u itself would put the whole
    tail of a narrow lobe, every theta_h beyond a2 samples[0], into the last one.  Not random, not differentiable, the same
    bits on every call."""
    if isinstance(size, bool) or not isinstance(size, int) or size < 2:
        raise ValueError('environment_brdf: size must be an int >= 2, got %r' % (size,))
    try:
        ny, nphi = (int(s) for s in samples)
    except (TypeError, ValueError):
        raise ValueError('environment_brdf: samples must be two positive ints (strata of y and of phi), got %r' % (samples,))
    if ny < 1 or nphi < 1:
        raise ValueError('environment_brdf: samples must be two positive ints (strata of y and of phi), got %r' % (samples,))
    f64 = torch.float64
    centres = (torch.arange(size, dtype=f64) + 0.5) / size
    span = 40.
    y = (((torch.arange(ny, dtype=f64) + 0.5) / ny * 2. - 1.) * span)[:, None]
    du = torch.sigmoid(y) * torch.sigmoid(-y) * (2. * span / ny)    # u (1 - u) dy
    phi = ((torch.arange(nphi, dtype=f64) + 0.5) / nphi * torch.pi)[None, :]
    nv = centres[None, None, :]                            # [1, 1, size]
    vx = torch.sqrt(1. - nv * nv)
    out = torch.empty((size, size, 2), dtype=f64)
    for i in range(size):
        rho = centres[i]
        a2 = (rho * rho) * (rho * rho)
        k = (rho + 1.) * (rho + 1.) / 8.
        tan2 = a2 * torch.exp(y)
        nh = torch.rsqrt(1. + tan2)
        sin_h = torch.sqrt(tan2) * nh
        hx = sin_h * torch.cos(phi)                        # [ny, nphi]; h = (hx, hy, nh), v = (vx, 0, nv): hy drops out of every product
        vh = hx[..., None] * vx + nh[..., None] * nv       # [ny, nphi, size]
        nl = 2. * vh * nh[..., None] - nv
        lit = (vh > 0) & (nl > 0)
        vis = 0.25 / ((nl * (1. - k) + k) * (nv * (1. - k) + k))
        w = torch.where(lit, 4. * vis * nl * vh / nh[..., None], torch.zeros((), dtype=f64)) * du[..., None]
        t = 1. - vh
        fc = ((t * t) * (t * t)) * t
        out[i, :, 0] = (w * (1. - fc)).mean(dim=1).sum(dim=0)
        out[i, :, 1] = (w * fc).mean(dim=1).sum(dim=0)
    return out.to(torch.float32)


def _table_lookup(table, row, col):
    """table [S, S, C], fractional indices row, col [...] inside it -> [..., C]: the bilinear blend of `texture.sample_cube`"""
    s = table.shape[0]
    fr0, fc0 = torch.floor(row), torch.floor(col)
    fr, fc = (row - fr0)[..., None], (col - fc0)[..., None]
    r, c = fr0.to(torch.int64), fc0.to(torch.int64)

    def fetch(rows, cols):
        return table[rows.clamp(0, s - 1), cols.clamp(0, s - 1)]

    return (fetch(r, c) * (1. - fc) * (1. - fr) + fetch(r, c + 1) * fc * (1. - fr)
            + fetch(r + 1, c) * (1. - fc) * fr + fetch(r + 1, c + 1) * fc * fr)


def image_based_lighting(vertex_positions, vertex_normals, vertex_colors, roughness, metalness, camera_position, pyramid_levels,
                         irradiance, brdf, intensity=(1., 1., 1.), min_roughness=0.04, dielectric_f0=0.04):
    """Metallic-roughness reflectance under an environment, by the split sum.
    positions, normals, colours (albedo) [*, V, 3]; roughness, metalness [*, V]; camera_position, intensity [*, 3];
    pyramid_levels: the L levels [6, n_k, n_k, 3] of a GGX-prefiltered environment (`texture.prefilter_cube(...).level(k)`,
    level k filtered at roughness k / (L - 1)); irradiance [6, M, M, 3] (`texture.convolve_cube(kind='lambert')`);
    brdf [S, S, 2] (`environment_brdf`) -> [*, V, 3].  Per point (every normalisation is torch.nn.functional.normalize,
    x / max(|x|, 1e-12); the cube look-ups are `texture.sample_cube(cube, *texture.directions_to_cube_indices(d, n))`):

        n^ = normalize(n)        v = normalize(cam - p)        nv_raw = n^ . v        nv = max(nv_raw, 0)
        rho = clamp(r, min_roughness, 1)                        F0_j = dielectric_f0 (1 - mu) + c_j mu
        R = 2 nv_raw n^ - v                                     (the view vector mirrored at n^; the unclamped product)
        (A, B) = bilinear look-up of brdf at col = clamp(nv S - 0.5, 0, S - 1), row = clamp(rho S - 0.5, 0, S - 1)
        S_j = F0_j A + B
        lam = rho (L - 1), l = floor(lam), f = lam - l:  spec_j = (1 - f) level_l(R) + f level_{l+1}(R)
        E_j = irradiance(n)                                     (the raw normal: an all-zero n is invalid and gives 0)
        L_j = intensity_j ((1 - S_j)(1 - mu) c_j E_j + S_j spec_j)

    The diffuse weight is (1 - S_j)(1 - mu): what the specular lobe reflects of a white environment is not available to the
    diffuse one.  Differentiable in everything but the table's use as an index; works in float64; min_roughness in (0, 1] and
    dielectric_f0 in [0, 1] are python numbers."""
    from .texture import directions_to_cube_indices, sample_cube
    min_roughness, dielectric_f0 = float(min_roughness), float(dielectric_f0)
    if not 0. < min_roughness <= 1.:
        raise ValueError('min_roughness must be > 0 and <= 1, got %r' % min_roughness)
    if not 0. <= dielectric_f0 <= 1.:
        raise ValueError('dielectric_f0 must lie in [0, 1], got %r' % dielectric_f0)
    levels = list(pyramid_levels)
    if not levels:
        raise ValueError('pyramid_levels must hold at least one level')
    p = _as(vertex_positions, torch.zeros((), dtype=torch.float32))
    n, c, r, mu, cam, inten = (_as(x, p) for x in (vertex_normals, vertex_colors, roughness, metalness, camera_position, intensity))
    table = _as(brdf, p)
    normalize = lambda x: torch.nn.functional.normalize(x, dim=-1, eps=1.e-12)   # noqa: E731
    nh_ = normalize(n)
    v = normalize(cam[..., None, :] - p)
    rho = torch.clamp(r, min_roughness, 1.)
    mu1 = mu[..., None]
    f0 = dielectric_f0 * (1. - mu1) + c * mu1
    nv_raw = torch.sum(nh_ * v, dim=-1)
    nv = torch.clamp(nv_raw, min=0.)
    refl = (2. * nv_raw)[..., None] * nh_ - v
    size = int(table.shape[0])
    ab = _table_lookup(table, (rho * float(size) - 0.5).clamp(0., float(size - 1)), (nv * float(size) - 0.5).clamp(0., float(size - 1)))
    s = f0 * ab[..., :1] + ab[..., 1:]
    top = float(len(levels) - 1)
    lam = torch.clamp(rho * top, 0., top)
    low = torch.floor(lam)
    f = (lam - low)[..., None]
    l0 = low.to(torch.int64)
    l1 = (l0 + 1).clamp(max=len(levels) - 1)
    looked = torch.stack([sample_cube(_as(lv, p), *directions_to_cube_indices(refl, int(lv.shape[1]))) for lv in levels])   # [L, *, V, 3]
    pick = lambda l: torch.gather(looked, 0, l[None, ..., None].expand((1,) + tuple(looked.shape[1:])))[0]   # noqa: E731
    spec = (1. - f) * pick(l0) + f * pick(l1)
    irr = _as(irradiance, p)
    e = sample_cube(irr, *directions_to_cube_indices(n, int(irr.shape[1])))
    return inten[..., None, :] * (((1. - s) * (1. - mu1)) * c * e + s * spec)


# ---- tangent-space normal mapping.  Not in the reference: per-vertex tangent frames from the uvs and the per-pixel frame
# that turns a normal-map texel into a shading normal.  These are the specifications `geometry.vertex_tangents` and
# `shading.perturb_normals` implement.

def _dot(a, b):
    return torch.sum(a * b, dim=-1, keepdim=True)


def _guarded_unit(x):
    """(x / |x| with a denominator of 1 where x is zero, so that no NaN reaches a gradient; [..., 1] bool: x . x > 0)"""
    xx = _dot(x, x)
    ok = xx > 0
    return x / torch.sqrt(torch.where(ok, xx, torch.ones_like(xx))), ok


def vertex_tangents(vertices, normals, uvs, faces):
    """Per-vertex tangent frames from the uv parametrisation: [*, V, 3|4], [*, V, 3], [V, 2], [F, 3] -> [*, V, 4], the unit
    tangent (the direction of increasing u, orthogonal to the normal) and the handedness w = -1 or +1 of the bitangent
    w * cross(n, t) against the direction of increasing v.  The normals are taken as given (unit, as `vertex_normals` returns
    them); the uvs are shared by the scenes and constant (no gradient).  Per face, with s = sign(det):

        e1 = p1 - p0, e2 = p2 - p0      (du1, dv1) = uv1 - uv0, (du2, dv2) = uv2 - uv0      det = du1 dv2 - du2 dv1
        t_f = s (dv2 e1 - dv1 e2)       b_f = s (du1 e2 - du2 e1)

    A face is live iff its det is finite and non-zero.  A dead face -- a degenerate uv triangle, a NaN or Inf uv -- has the
    four coefficients s dv2, s dv1, s du1, s du2 exactly 0: it adds nothing to T, Bt or any gradient, whatever its uvs hold.

    Per vertex, T and Bt the sums of t_f and b_f over the faces that name it (once per naming corner):

        x = T - n (n . T)       t = x / |x| where x . x > 0, else 0       w = -1 where cross(n, t) . Bt < 0, else +1

    w carries no gradient, and so neither does Bt."""
    vertices, faces = _prepare_vertices_and_faces(vertices, faces)
    p = vertices[..., :3]
    n = _as(normals, p)
    uv = _as(uvs, p).detach()
    p0, p1, p2 = (p[..., faces[:, k], :] for k in range(3))
    e1, e2 = p1 - p0, p2 - p0
    d1, d2 = uv[faces[:, 1]] - uv[faces[:, 0]], uv[faces[:, 2]] - uv[faces[:, 0]]
    du1, dv1, du2, dv2 = d1[:, 0:1], d1[:, 1:2], d2[:, 0:1], d2[:, 1:2]
    det = du1 * dv2 - du2 * dv1
    live = torch.isfinite(det) & (det != 0)
    s, zero = torch.sign(det), torch.zeros_like(det)
    a, b, c, d = (torch.where(live, s * x, zero) for x in (dv2, dv1, du1, du2))     # (a select: 0 * NaN would be NaN)
    t_f = a * e1 - b * e2
    b_f = c * e2 - d * e1
    T, Bt = torch.zeros_like(p), torch.zeros_like(p)
    for k in range(3):
        T = T.index_add(-2, faces[:, k], t_f)
        Bt = Bt.index_add(-2, faces[:, k], b_f.detach())
    t, _ = _guarded_unit(T - n * _dot(n, T))
    w = torch.where(_dot(torch.linalg.cross(n, t, dim=-1), Bt) < 0, -1., 1.).to(t.dtype).detach()
    return torch.cat([t, w], dim=-1)


def perturb_normals(normals, tangents, normal_map, strength=1.0, encoded=True):
    """The shading normal of a tangent-space normal map: [*, 3], [*, 4] (`vertex_tangents`, interpolated), [*, 3] -> [*, 3].

        d = 2 normal_map - 1 if encoded, else normal_map;  d.xy *= strength  (a python number, no gradient)
        N = n / |n|       x = t - N (N . t),  T = x / |x|       Bv = w cross(N, T)
        y = d.x T + d.y Bv + d.z N        out = y / |y|

    where n . n > 0, x . x > 0 and y . y > 0; any other element -- a background's zero normal, a zero tangent, a tangent
    parallel to the normal, a zero decoded vector -- returns its normal unchanged and passes the incoming gradient to it
    alone.  w multiplies as given (an interpolated handedness is a weight) and receives its gradient."""
    n = _as(normals, torch.zeros((), dtype=torch.float32))
    tangents, m = _as(tangents, n), _as(normal_map, n)
    t, w = tangents[..., :3], tangents[..., 3:4]
    d = 2. * m - 1. if encoded else m
    dx, dy, dz = d[..., 0:1] * float(strength), d[..., 1:2] * float(strength), d[..., 2:3]
    N, ok_n = _guarded_unit(n)
    T, ok_x = _guarded_unit(t - N * _dot(N, t))
    Bv = w * torch.linalg.cross(N, T, dim=-1)
    out, ok_y = _guarded_unit((dx * T + dy * Bv) + dz * N)
    return torch.where(ok_n & ok_x & ok_y, out, n)


# ---- shadow maps.  Not in the reference: the per-point look-up of a depth image rendered from a light (`shading.render_shadow_map`)
# with a percentage-closer filter and a smooth comparison, so that the visibility is differentiable in the point, in the map and in
# the light's matrix.  This is the specification `shading.shadow_visibility` implements per pixel.

SHADOW_MAX_LIGHTS = 4
SHADOW_KERNELS = (1, 3, 5)


def shadow_visibility(points, normals, shadow_maps, light_matrices, *, mask=None, kernel=3, bias=0.0, softness, normal_offset=0.0):
    """The share of each light that reaches each point, from the lights' depth maps: points [N, 3] (world space), normals [N, 3]
    or None (needed only with normal_offset != 0), shadow_maps [L, Hs, Ws] (clip-space z of the nearest surface, as
    `shading.render_shadow_map` draws it), light_matrices [L, 4, 4] (world -> the light's clip space, right-multiplying row
    vectors as everything in `matrices`), mask [N] or None -> [N, L], 1 = lit, 0 = in shadow.  kernel (1, 3 or 5), bias,
    softness (> 0, and no smaller than 2.94e-39: its float32 reciprocal must be finite) and normal_offset are python numbers
    and carry no gradient.  Per point and light:

        q = p + normal_offset n / max(|n|, 1e-12)                    (x, y, z, w) = [q, 1] @ M            d = z
        col = (x / w + 1) Ws / 2 - 0.5          row = (1 - y / w) Hs / 2 - 0.5
            (the fractional texel-centre indices of the image `rasterise` draws with M: row 0 is the top, window y = Hs - 0.5)
        h = (kernel - 1) / 2      r0 = floor(row) - h,  fr = row - floor(row)      c0 = floor(col) - h,  fc = col - floor(col)
        wr[0] = 1 - fr,  wr[kernel] = fr,  wr[a] = 1 between; wc likewise with fc
        S(r, c) = s((Z[r, c] - d + bias) / softness + 1/2) for a texel of the map,  1 for one outside it
        s(t) = u u (3 - 2 u),  u = clamp(t, 0, 1)
        v = (1 / kernel^2) sum_{a, b = 0..kernel} wr[a] wc[b] S(r0 + a, c0 + b)
        out = 1 - m (1 - v)

    v is the mean of kernel^2 bilinear blends of the comparison S, at the texel offsets -h .. h, written as one window of
    (kernel + 1)^2 texels.  A point that is not in front of the light (not w > 0, a NaN included) or whose whole window lies
    off the map has v = 1 and no gradient, and adds none to the matrix either; a texel outside the map receives none.  floor and the inside tests carry no
    gradient; the clamp passes none outside (0, 1) (and s' is 0 at both ends)."""
    kernel, bias, softness, normal_offset = _shadow_scalars(kernel, bias, softness, normal_offset)
    p = _as(points, torch.zeros((), dtype=torch.float32))
    maps, mats = _as(shadow_maps, p), _as(light_matrices, p)
    if p.dim() != 2 or p.shape[1] != 3:
        raise ValueError('points must have shape [N, 3], got %s' % (tuple(p.shape),))
    if maps.dim() != 3 or not 1 <= maps.shape[0] <= SHADOW_MAX_LIGHTS or 0 in maps.shape:
        raise ValueError('shadow_maps must have shape [L, Hs, Ws] with 1 <= L <= %d, got %s' % (SHADOW_MAX_LIGHTS, tuple(maps.shape)))
    if tuple(mats.shape) != (maps.shape[0], 4, 4):
        raise ValueError('light_matrices must have shape [%d, 4, 4], got %s' % (maps.shape[0], tuple(mats.shape)))
    q = p
    if normal_offset != 0.:
        if normals is None:
            raise ValueError('normal_offset needs normals')
        q = p + normal_offset * torch.nn.functional.normalize(_as(normals, p), dim=-1, eps=1.e-12)
    finite = torch.isfinite(q).all(dim=1)
    q = torch.where(finite[:, None], q, torch.zeros_like(q))   # (a select: the matrix's gradient is q^T d clip, and NaN * 0 would be NaN)
    L, Hs, Ws = (int(s) for s in maps.shape)
    h = (kernel - 1) // 2
    taps = torch.arange(kernel + 1, device=p.device)
    one = torch.ones_like(q[:, 0])
    out = []
    for l in range(L):
        M = mats[l]
        x, y, d, w = (((q[:, 0] * M[0, j] + q[:, 1] * M[1, j]) + q[:, 2] * M[2, j]) + M[3, j] for j in range(4))
        # (a finite point that x or y overflow on is off every map; kept out of x / w, whose backward would make 0 * Inf of it)
        front = finite & (w > 0) & torch.isfinite(x) & torch.isfinite(y)
        ws = torch.where(front, w, one)
        col = (x / ws + 1.) * (0.5 * Ws) - 0.5
        row = (1. - y / ws) * (0.5 * Hs) - 0.5
        fr0, fc0 = torch.floor(row.detach()), torch.floor(col.detach())
        on = front & (fr0 + (h + 1) >= 0) & (fr0 - h <= Hs - 1) & (fc0 + (h + 1) >= 0) & (fc0 - h <= Ws - 1)
        zero = torch.zeros_like(row)
        row, col, fr0, fc0 = torch.where(on, row, zero), torch.where(on, col, zero), torch.where(on, fr0, zero), torch.where(on, fc0, zero)
        fr, fc = row - fr0, col - fc0
        r = (fr0.long() - h)[:, None] + taps
        c = (fc0.long() - h)[:, None] + taps
        inside = ((r >= 0) & (r < Hs))[:, :, None] & ((c >= 0) & (c < Ws))[:, None, :]
        Z = maps[l][r.clamp(0, Hs - 1)[:, :, None], c.clamp(0, Ws - 1)[:, None, :]]
        u = torch.clamp(((Z - d[:, None, None]) + bias) / softness + 0.5, 0., 1.)
        S = torch.where(inside, (u * u) * (3. - 2. * u), torch.ones_like(u))
        middle = [one] * (kernel - 1)
        wr, wc = torch.stack([1. - fr] + middle + [fr], dim=1), torch.stack([1. - fc] + middle + [fc], dim=1)
        v = torch.sum(wr[:, :, None] * wc[:, None, :] * S, dim=(1, 2)) * (1. / (kernel * kernel))
        out.append(torch.where(on, v, one))
    v = torch.stack(out, dim=1)
    if mask is None:
        return v
    return 1. - _as(mask, p)[:, None] * (1. - v)


def _shadow_scalars(kernel, bias, softness, normal_offset):
    """The four python numbers of `shadow_visibility`, refused outside their ranges -> (kernel, bias, softness, normal_offset)."""
    if isinstance(kernel, bool) or kernel not in SHADOW_KERNELS:
        raise ValueError('kernel must be 1, 3 or 5, got %r' % (kernel,))
    for name, x in (('bias', bias), ('softness', softness), ('normal_offset', normal_offset)):
        if isinstance(x, bool) or not isinstance(x, numbers.Real) or not math.isfinite(x):
            raise ValueError('%s must be a finite number, got %r' % (name, x))
    if not softness > 0:
        raise ValueError('softness must be > 0, got %r' % (softness,))
    # the kernel multiplies by the float32 reciprocal: below 1 / FLT_MAX (2.94e-39) that is Inf, and 0 * Inf a NaN
    as_float32 = ctypes.c_float(softness).value
    if as_float32 == 0. or 1. / as_float32 > (2. - 2.**-23) * 2.**127:
        raise ValueError('softness must have a finite float32 reciprocal, got %r' % (softness,))
    return int(kernel), float(bias), float(softness), float(normal_offset)


# ---- the environment behind the mesh.  Not in the reference: the pixels a mesh does not cover show the environment cube, looked
# up along the ray through the pixel's centre, at a level of detail that follows from the camera alone.  This is the specification
# `shading.environment_background` implements per pixel.

BACKGROUND_FILTERS = ('nearest', 'bilinear', 'trilinear')


def _image_size(size):
    """An image's size as the shadow maps and the background take it: a positive int or (height, width) -> (height, width)."""
    try:
        hs, ws = (size, size) if isinstance(size, numbers.Integral) else size
        ok = all(isinstance(s, numbers.Integral) and not isinstance(s, bool) and s >= 1 for s in (hs, ws))
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError('size must be a positive int or (height, width), got %r' % (size,))
    return int(hs), int(ws)


def _background_scalars(size, filter, lod, lod_bias, max_level):
    """The python arguments of `environment_background`, refused outside their ranges -> (height, width, lod or None, lod_bias)."""
    height, width = _image_size(size)
    if filter not in BACKGROUND_FILTERS:
        raise ValueError("environment_background: filter must be 'nearest', 'bilinear' or 'trilinear', got %r" % (filter,))
    if filter != 'trilinear' and (lod is not None or lod_bias != 0.0 or max_level is not None):
        raise ValueError("lod, lod_bias and max_level apply to filter='trilinear' only (got filter=%r)" % (filter,))
    if max_level is not None and (isinstance(max_level, bool) or not isinstance(max_level, int) or max_level < 0):
        raise ValueError('max_level must be a non-negative int or None, got %r' % (max_level,))
    for name, x in (('lod', lod), ('lod_bias', lod_bias)):
        if x is not None and (isinstance(x, bool) or not isinstance(x, numbers.Real) or not math.isfinite(x)):
            raise ValueError('%s must be a finite number%s, got %r' % (name, ' or None (the footprint of the pixel)' if name == 'lod' else '', x))
    return height, width, None if lod is None else float(lod), float(lod_bias)


def _box_levels(cube, max_level):
    """The box-filtered levels of a cube [6, N, N, C], as `texture.cube_pyramid` makes them: 2 x 2 means while the size is even."""
    levels = [cube]
    while levels[-1].shape[1] % 2 == 0 and (max_level is None or len(levels) <= max_level):
        t = levels[-1]
        levels.append(((t[:, 0::2, 0::2] + t[:, 0::2, 1::2]) + (t[:, 1::2, 0::2] + t[:, 1::2, 1::2])) * 0.25)
    return levels


def background_rays(clip_to_world, height, width):
    """The rays through the pixel centres of a height x width image, one operation per step as `environment_background` states
    them: clip_to_world [..., 4, 4] -> dict of nx, ny [height, width], h0, hm (lists of four [..., height, width]: the
    homogeneous world points on the planes z = 0 and z = -1 of clip space)."""
    M = clip_to_world
    two = torch.full((), 2., dtype=M.dtype, device=M.device)
    nx = (two * (torch.arange(width, dtype=M.dtype, device=M.device) + 0.5)) / float(width) - 1.
    ny = 1. - (two * (torch.arange(height, dtype=M.dtype, device=M.device) + 0.5)) / float(height)
    nx, ny = nx[None, :].expand(height, width), ny[:, None].expand(height, width)
    Mb = M[..., None, None, :, :]
    a = [nx * Mb[..., 0, j] + ny * Mb[..., 1, j] for j in range(4)]
    return {'nx': nx, 'ny': ny, 'h0': [a[j] + Mb[..., 3, j] for j in range(4)], 'hm': [(a[j] - Mb[..., 2, j]) + Mb[..., 3, j] for j in range(4)]}


def _background_footprint(M, rays, start, end, d, size, height, width):
    """log2 of a pixel's footprint in texels of level 0, from the camera alone (no gradient): the derivative of the ray by the
    pixel's column and row in closed form, through the face coordinates of d's own face."""
    x, y, z = d.unbind(-1)
    ax, ay, az = x.abs(), y.abs(), z.abs()
    is_x = (ax >= ay) & (ax >= az)
    is_y = ~is_x & (ay >= az)
    major = torch.where(is_x, x, torch.where(is_y, y, z))
    pos = major > 0
    a = torch.where(is_x, ax, torch.where(is_y, ay, az))
    a = torch.where(a > 0, a, torch.ones_like(a))

    def picks(v):   # (sc, tc, the major component times its sign) of the vector v on d's face
        vx, vy, vz = v
        sc = torch.where(is_x, torch.where(pos, -vz, vz), torch.where(is_y, vx, torch.where(pos, vx, -vx)))
        tc = torch.where(is_y, torch.where(pos, vz, -vz), -vy)
        mc = torch.where(is_x, vx, torch.where(is_y, vy, vz))
        return sc, tc, torch.where(pos, mc, -mc)

    sc, tc, _ = picks((x, y, z))
    s, t = sc / a, tc / a
    Mb = M[..., None, None, :, :]
    h0w, hmw = rays['h0'][3], rays['hm'][3]
    n2 = []
    for axis, n in ((0, width), (1, height)):
        scale = torch.full((), 2., dtype=M.dtype, device=M.device) / float(n)
        row = [Mb[..., axis, j] for j in range(4)]
        dd = [scale * ((row[j] - end[..., j] * row[3]) / h0w - (row[j] - start[..., j] * row[3]) / hmw) for j in range(3)]
        dsc, dtc, dma = picks(dd)
        ds, dt = (dsc - s * dma) / a, (dtc - t * dma) / a
        n2.append(ds * ds + dt * dt)
    big = torch.where(n2[0] > n2[1], n2[0], n2[1])
    return torch.log2((0.5 * float(size)) * torch.sqrt(big))


def environment_background(environment, clip_to_world, size, *, mask=None, intensity=(1., 1., 1.), filter='bilinear', lod=None, lod_bias=0.0,
                           max_level=None):
    """The environment as a camera sees it where no mesh covers the pixel.  environment: a cube [6, N, N, 3] (faces +X, -X, +Y,
    -Y, +Z, -Z as `texture.sample_cube` takes them) or a 3-channel `texture.CubePyramid` (filter='trilinear' only); clip_to_world
    [4, 4] or [B, 4, 4], what `projection.unproject_pixels_to_rays` takes (row vectors, typically inverse(view @ projection));
    size: an int or (height, width); mask None or [H, W] / [B, H, W], 1 where the mesh covers the pixel; intensity 3 numbers,
    [3] or [B, 3] -> [H, W, 3] or [B, H, W, 3].  Per pixel (r, c), one operation per step:

        nx = (2 (c + 0.5)) / W - 1              ny = 1 - (2 (r + 0.5)) / H         (projection._pixel_to_ndc at the pixel centre)
        a_j = nx M[0][j] + ny M[1][j]           h0_j = a_j + M[3][j]               hm_j = (a_j - M[2][j]) + M[3][j]
        end = h0.xyz / h0.w                     start = hm.xyz / hm.w              d = end - start
            (the second result of `unproject_pixels_to_rays` at the pixel centres, not normalised)
        E = `texture.sample_cube(level, *texture.directions_to_cube_indices(d, n))`: 'nearest', 'bilinear', or 'trilinear':
            lam = clamp(lambda, 0, L - 1), l = floor(lam), f = lam - l:  E = (1 - f) level_l(d) + f level_{l+1}(d)
        out_j = ((1 - m) intensity_j) E_j

    lambda is `lod` + `lod_bias`, or with lod=None the pixel's own footprint: with dd_x = (2 / W) d d / d nx and dd_y = (2 / H)
    d d / d ny in closed form (d end / d nx = (M[0].xyz - end M[0].w) / h0.w, start likewise with hm; ny with M[1]),

        Ds = (sc(dd) - s ma(dd)) / a            Dt = (tc(dd) - t ma(dd)) / a       (d's own face: its picks of dd; s, t, a of d)
        rho = (N / 2) sqrt(max(Ds_x^2 + Dt_x^2, Ds_y^2 + Dt_y^2))                  lambda = log2 rho + lod_bias

    held constant: no gradient flows through it.  A pixel whose d is not valid (h.w = 0, anything non-finite, all zero) or whose
    1 - m is exactly 0 gives 0 and takes part in no gradient but the mask's.  With 'trilinear' a cube's levels are its 2 x 2 box
    means (`texture.cube_pyramid`, capped by max_level).  Differentiable in the environment, the matrix, the intensity and the
    mask; works in float64 and on any device."""
    from .texture import CubePyramid, directions_to_cube_indices, sample_cube
    height, width, lod, lod_bias = _background_scalars(size, filter, lod, lod_bias, max_level)
    if isinstance(environment, CubePyramid):
        if filter != 'trilinear':
            raise ValueError("environment_background: a CubePyramid is looked up with filter='trilinear', got %r" % (filter,))
        levels = [environment.level(k) for k in range(environment.levels)]
    else:
        levels = _box_levels(environment, max_level) if filter == 'trilinear' else [environment]
    like = levels[0]
    if like.dim() != 4 or like.shape[0] != 6 or like.shape[1] != like.shape[2] or like.shape[3] != 3:
        raise ValueError('environment must be a cube [6, size, size, 3], got %s' % (tuple(like.shape),))
    M, inten = _as(clip_to_world, like), _as(intensity, like)
    m = None if mask is None else _as(mask, like)
    if M.dim() not in (2, 3) or tuple(M.shape[-2:]) != (4, 4):
        raise ValueError('clip_to_world must have shape [4, 4] or [B, 4, 4], got %s' % (tuple(M.shape),))
    if inten.dim() not in (1, 2) or inten.shape[-1] != 3:
        raise ValueError('intensity must have shape [3] or [B, 3], got %s' % (tuple(inten.shape),))
    if m is not None and (m.dim() not in (2, 3) or tuple(m.shape[-2:]) != (height, width)):
        raise ValueError('mask must have shape [%d, %d] or [B, %d, %d], got %s' % (height, width, height, width, tuple(m.shape)))
    n = int(like.shape[1])
    w = None if m is None else 1. - m
    rays = background_rays(M, height, width)
    with torch.no_grad():
        raw = torch.stack([rays['h0'][j] / rays['h0'][3] - rays['hm'][j] / rays['hm'][3] for j in range(3)], -1)
        valid = torch.isfinite(raw).all(-1) & (raw.abs().amax(-1) > 0)
        if w is not None:
            valid = valid & (w != 0)
    # (selects: a pixel that is not valid keeps 0 / 1 in place of its ray, so that no Inf or NaN meets a zero in a backward)
    zero, one = torch.zeros_like(rays['h0'][3]), torch.ones_like(rays['h0'][3])
    valid = valid.expand(torch.broadcast_shapes(valid.shape, zero.shape))
    h0w, hmw = torch.where(valid, rays['h0'][3], one), torch.where(valid, rays['hm'][3], one)
    end = torch.stack([torch.where(valid, rays['h0'][j], zero) / h0w for j in range(3)], -1)
    start = torch.stack([torch.where(valid, rays['hm'][j], zero) / hmw for j in range(3)], -1)
    d = end - start
    mode = 'nearest' if filter == 'nearest' else 'bilinear'
    if filter != 'trilinear':
        E = sample_cube(like, *directions_to_cube_indices(d, n), mode)
    else:
        with torch.no_grad():
            if lod is None:
                safe = dict(rays, h0=rays['h0'][:3] + [h0w], hm=rays['hm'][:3] + [hmw])
                lam = _background_footprint(M, safe, start, end, d, n, height, width) + lod_bias
            else:
                lam = (torch.full((), lod, dtype=like.dtype, device=like.device) + lod_bias).expand(d.shape[:-1])
            top = float(len(levels) - 1)
            lam = torch.where(lam > 0, torch.where(lam < top, lam, torch.full_like(lam, top)), torch.zeros_like(lam))   # (a NaN: level 0)
            low = torch.floor(lam)
            f = (lam - low)[..., None]
            l0 = low.to(torch.int64)
            l1 = (l0 + 1).clamp(max=len(levels) - 1)
        looked = torch.stack([sample_cube(lv, *directions_to_cube_indices(d, int(lv.shape[1]))) for lv in levels])   # [L, ..., H, W, 3]
        pick = lambda l: torch.gather(looked, 0, l[None, ..., None].expand((1,) + tuple(looked.shape[1:])))[0]   # noqa: E731
        E = torch.where(f != 0, (1. - f) * pick(l0) + f * pick(l1), pick(l0))
    scale = inten[..., None, None, :] if w is None else w[..., None] * inten[..., None, None, :]
    out = scale * E
    return torch.where(valid[..., None], out, torch.zeros_like(out))


# ---- the developed image: supersample resolve, exposure, tone curve, sRGB encode, clamp

RESOLVE_CURVES = ('linear', 'reinhard', 'aces')
RESOLVE_ENCODINGS = ('linear', 'srgb')
RESOLVE_MAX_FACTOR, RESOLVE_MAX_CHANNELS = 4, 4
SRGB_KNEE = 0.0031308   # the linear value where the sRGB transfer function leaves its linear segment


def srgb_encode(x):
    """The sRGB transfer function of a linear value, per element: u = max(x, 0); 12.92 u where u <= 0.0031308, else
    1.055 u^(1 / 2.4) - 0.055.  (The power is taken of max(u, knee): the branch that is not taken cannot put inf * 0 into a gradient.)"""
    u = x.clamp_min(0.)
    return torch.where(u <= SRGB_KNEE, 12.92 * u, 1.055 * u.clamp_min(SRGB_KNEE) ** (1. / 2.4) - 0.055)


def srgb_decode(y):
    """The inverse of `srgb_encode` on [0, 1], which linearises a photograph: y / 12.92 where y <= 12.92 * 0.0031308, else
    ((y + 0.055) / 1.055)^2.4."""
    knee = 12.92 * SRGB_KNEE
    return torch.where(y <= knee, y / 12.92, ((y.clamp_min(knee) + 0.055) / 1.055) ** 2.4)


def _resolve_scalars(factor, curve, white, encode, clamp):
    """The python arguments of `resolve_image`, refused outside their ranges -> (lo, hi) of the clamp or None."""
    if isinstance(factor, bool) or not isinstance(factor, numbers.Integral) or not 1 <= factor <= RESOLVE_MAX_FACTOR:
        raise ValueError('resolve_image: factor must be an int in 1..%d, got %r' % (RESOLVE_MAX_FACTOR, factor))
    if curve not in RESOLVE_CURVES:
        raise ValueError("resolve_image: curve must be 'linear', 'reinhard' or 'aces', got %r" % (curve,))
    if encode not in RESOLVE_ENCODINGS:
        raise ValueError("resolve_image: encode must be 'linear' or 'srgb', got %r" % (encode,))
    if (curve == 'reinhard') != (white is not None):
        raise ValueError("resolve_image: white goes with curve='reinhard' and only with it (got curve=%r, white=%r)" % (curve, white))
    if white is not None and not isinstance(white, torch.Tensor) and (isinstance(white, bool) or not isinstance(white, numbers.Real) or not white > 0):
        raise ValueError('resolve_image: white must be a positive number or a tensor, got %r' % (white,))
    if clamp is None:
        return None
    try:
        lo, hi = (float(v) for v in clamp)
    except (TypeError, ValueError):
        raise ValueError('clamp must be (lo, hi) or None, got %r' % (clamp,))
    if not lo <= hi:
        raise ValueError('clamp needs lo <= hi, got %r' % (clamp,))
    return lo, hi


def _resolve_sizes(image, factor):
    """Refuses an image that `resolve_image` cannot resolve by its shape -> (H, W, C) of the output."""
    if not isinstance(image, torch.Tensor) or image.dim() not in (3, 4):
        raise ValueError('resolve_image expects image [S H, S W, C] or [B, S H, S W, C], got %s' % (tuple(getattr(image, 'shape', ())),))
    rows, cols, channels = (int(s) for s in image.shape[-3:])
    if not 1 <= channels <= RESOLVE_MAX_CHANNELS:
        raise ValueError('resolve_image: image has %d channels, 1..%d' % (channels, RESOLVE_MAX_CHANNELS))
    if rows % factor or cols % factor:
        raise ValueError('resolve_image: an image of %d x %d samples is no multiple of factor=%d each way' % (rows, cols, factor))
    return rows // factor, cols // factor, channels


def resolve_image(image, *, add=None, factor=1, exposure=1.0, curve='linear', white=None, encode='linear', clamp=(0., 1.)):
    """What every rendered image goes through between the shaders and a loss against a photograph: two radiance images added,
    S x S samples box-filtered into a pixel, exposure, a tone curve, the sRGB transfer function, a clamp.  image
    [S H, S W, C] or [B, S H, S W, C] with C in 1..4 and S = `factor` (1..4); add: None or a second image of the same shape;
    exposure: the gain per channel, a number, C numbers or a tensor [C] or [B, C] (exposure and white balance in one);
    curve 'linear', 'reinhard' (extended Reinhard, with the white point `white`: a positive number or a tensor [] or [B]) or
    'aces' (the Narkowicz fit); encode 'linear' or 'srgb'; clamp (lo, hi) or None -> [H, W, C] or [B, H, W, C].  Per output
    pixel (r, c) and channel ch, one operation per step and in this order:

        acc = 0;  for i in 0..S-1, for j in 0..S-1:  acc += image[S r + i, S c + j, ch] + add[S r + i, S c + j, ch]
        L = acc * (1 / S^2)                     E = exposure[ch] * L
        'linear':    t = E                      (negatives pass: masks and auxiliary channels resolve with the same call)
        otherwise    x = max(E, 0), and
        'reinhard':  t = x * (1 + x / (w * w)) / (1 + x)
        'aces':      t = x * (2.51 x + 0.03) / (x * (2.43 x + 0.59) + 0.14)
        'linear':    y = t
        'srgb':      u = max(t, 0);  y = 12.92 u where u <= 0.0031308, else 1.055 u^(1 / 2.4) - 0.055       (`srgb_encode`)
        out = clamp(y, lo, hi)

    A NaN stays NaN throughout.  Differentiable in image, add, exposure and white; works in float64 and on any device.  The
    sums are the explicit i, j loop, so that their order is the one `shading.resolve_image` keeps."""
    bounds = _resolve_scalars(factor, curve, white, encode, clamp)
    _resolve_sizes(image, factor)
    if add is not None and (not isinstance(add, torch.Tensor) or add.shape != image.shape):
        raise ValueError('resolve_image: add must have the shape of image, %s, got %s' % (tuple(image.shape), tuple(getattr(add, 'shape', ()))))
    S = int(factor)
    acc = torch.zeros_like(image[..., 0::S, 0::S, :])
    for i in range(S):
        for j in range(S):
            sample = image[..., i::S, j::S, :]
            acc = acc + (sample if add is None else sample + add[..., i::S, j::S, :])
    L = acc * torch.full((), 1. / (S * S), dtype=image.dtype, device=image.device)
    e = _as(exposure, image)
    if e.dim() == 2:
        e = e[:, None, None, :]
    E = e * L
    if curve == 'linear':
        t = E
    else:
        x = E.clamp_min(0.)
        if curve == 'reinhard':
            w = _as(white, image)
            if w.dim() == 1:
                w = w[:, None, None, None]
            t = x * (1. + x / (w * w)) / (1. + x)
        else:
            t = x * (2.51 * x + 0.03) / (x * (2.43 * x + 0.59) + 0.14)
    y = srgb_encode(t) if encode == 'srgb' else t
    return y if bounds is None else y.clamp(*bounds)
