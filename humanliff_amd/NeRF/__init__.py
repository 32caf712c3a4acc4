from .renderer import Renderer, render, render_rays, render_view  # noqa: F401
from .raster import rasterize  # noqa: F401
from .simplify import simplify_mesh  # noqa: F401
from .distance import mesh_distance, point_mesh_distance, sample_surface  # noqa: F401
