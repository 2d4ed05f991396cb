"""``chroma-render``: a headless picture of a geometry, written as a PNG.

The camera is placed as chroma/camera.py:117-136 places it (on the -y side of the mesh's bounding box, one diagonal away,
looking along +y with z up, a 35 mm film at 18 mm).  Without ``--hybrid`` the picture is GPURays.render's (the
surfaces' colours, composited over ``--alpha-depth`` layers); with it, the camera's hybrid mode (GPUHybridRender): the
geometry lit by a point source with its real optics, ``--lookups`` lookup passes and ``--images`` image passes.
"""
import argparse
import sys

import numpy as np


def _triple(text):
    v = [float(x) for x in text.split(',')]
    if len(v) != 3:
        raise argparse.ArgumentTypeError('expected X,Y,Z')
    return v


def _size(text):
    v = [int(x) for x in text.split(',')]
    if len(v) != 2 or min(v) < 1:
        raise argparse.ArgumentTypeError('expected W,H')
    return v


def camera_rays(geometry, size, film_width=35.0):
    """(point, positions, directions) of the camera's initial view of ``geometry`` (chroma/camera.py:117-136)."""
    from chroma_amd.tools import from_film
    lower, upper = geometry.mesh.get_bounds()
    diagonal = np.linalg.norm(upper - lower)
    point = np.array([(lower[0] + upper[0]) / 2, -diagonal, (lower[2] + upper[2]) / 2])
    pos, dirs = from_film(point, axis1=np.array([0, 0, 1], float), axis2=np.array([1, 0, 0], float), size=tuple(size),
                          width=film_width)
    return point, pos, dirs


def main(argv=None):
    ap = argparse.ArgumentParser(prog='chroma-render', description=__doc__.split('\n\n')[0])
    ap.add_argument('geometry', help='geometry string, as chroma-sim takes (e.g. "@chroma_amd.demo.tiny")')
    ap.add_argument('-r', '--resolution', type=_size, default=[800, 600], help='W,H (default 800,600)')
    ap.add_argument('--hybrid', action='store_true', help='light the geometry from a point source (the camera\'s hybrid mode)')
    ap.add_argument('--source', type=_triple, default=None, help='X,Y,Z of the point source (default: the camera position)')
    ap.add_argument('--lookups', type=int, default=1, help='lookup passes (default 1)')
    ap.add_argument('--images', type=int, default=1, help='image passes (default 1)')
    ap.add_argument('--max-steps', type=int, default=10, help='photon steps to the first diffuse reflection (default 10)')
    ap.add_argument('-s', '--seed', type=int, default=None, help='random seed of the hybrid mode')
    ap.add_argument('--alpha-depth', type=int, default=10, help='layers composited without --hybrid (default 10)')
    ap.add_argument('-j', '--device', type=int, default=0, help='GPU')
    ap.add_argument('-o', '--output', required=True, help='PNG file to write')
    args = ap.parse_args(argv)
    if args.lookups < 1 or args.images < 1 or args.max_steps < 0 or args.alpha_depth < 1:
        ap.error('--lookups and --images must be at least 1, --max-steps non-negative, --alpha-depth at least 1')

    from chroma_amd import gpu
    from chroma_amd.gpu.render import write_png
    from chroma_amd.loader import load_geometry_from_string
    gpu.create_cuda_context(args.device)
    geometry = load_geometry_from_string(args.geometry, cuda_device=args.device)
    width, height = args.resolution
    point, pos, dirs = camera_rays(geometry, (width, height))
    gpu_geometry = gpu.GPUGeometry(geometry)
    rays = gpu.GPURays(pos, dirs, max_alpha_depth=args.alpha_depth)
    if args.hybrid:
        source = point if args.source is None else np.asarray(args.source, float)
        renderer = gpu.GPUHybridRender(gpu_geometry, rays, seed=args.seed, max_steps=args.max_steps)
        pixels = renderer.snapshot(source, nlookup=args.lookups, nimages=args.images)
    else:
        pixels = rays.snapshot(gpu_geometry, alpha_depth=args.alpha_depth)
    write_png(args.output, pixels, width, height)
    return 0


if __name__ == '__main__':
    sys.exit(main())
