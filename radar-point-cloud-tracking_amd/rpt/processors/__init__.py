"""Drop-in for ``radar_pipeline.processors`` (hot-path members only)."""
from .cartesian import (  # noqa: F401
    aligned_inputs,
    convert_batch_aligned,
    convert_single_csv,
)
from .clustering import (  # noqa: F401
    cluster_point_cloud,
    infer_time_from_colors,
    neighbour_counts,
    process_ply_clustering,
    st_dbscan,
    st_dbscan_sweep,
)
from .point_cloud import (  # noqa: F401
    build_stacked_clouds,
    combine_clouds,
    find_gain_sweeps,
    load_points_from_csv,
)
