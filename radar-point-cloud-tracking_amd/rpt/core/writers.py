"""Drop-in for ``radar_pipeline.core.writers.write_ply`` and ``write_labels_csv``
(core/writers.py:13-46, :65-81).  The text rows of both are formed on the device when one is
visible (rpt/core/text.py, csrc/text.hip) and by the reference's own expressions otherwise; the
bytes written are the same either way."""
from __future__ import annotations

from pathlib import Path

import numpy as np

from .loaders import PointCloud


def write_ply(path: Path, cloud: PointCloud) -> None:
    """writers.py:13-46: ASCII PLY with uchar RGB, grey 180 without colours.  The members of
    ``cloud`` may be numpy arrays or torch tensors (device tensors are formatted where they
    are and reach the file through a pinned buffer)."""
    from . import text

    path = Path(path)
    num_points = cloud.size
    colors = cloud.colors
    if colors is None:
        colors = np.full((num_points, 3), 180, dtype=np.uint8)
    header = ("ply\n"
              "format ascii 1.0\n"
              f"element vertex {num_points}\n"
              "property float x\n"
              "property float y\n"
              "property float z\n"
              "property uchar red\n"
              "property uchar green\n"
              "property uchar blue\n"
              "end_header\n")
    path.parent.mkdir(parents=True, exist_ok=True)
    with path.open("wb") as fh:
        fh.write(header.encode("utf-8"))
        text.write_text(fh, text.format_ply_rows(cloud.x, cloud.y, cloud.z, colors,
                                                     as_tensor=True))


def write_labels_csv(path: Path, coords: np.ndarray, labels: np.ndarray) -> None:
    """writers.py:65-81.  (N, 3) float32 coordinates with int32-range integer labels go through
    the device formatter when a GPU is visible; everything else is np.savetxt as before."""
    from . import text

    path = Path(path)
    path.parent.mkdir(parents=True, exist_ok=True)
    c = np.asarray(coords)
    lab = np.asarray(labels)
    if (text.gpu_visible() and c.ndim == 2 and c.shape[1] == 3 and c.dtype == np.float32
            and lab.ndim == 1 and lab.dtype.kind in "iu" and len(lab) == len(c)):
        rows = text.format_label_rows(c[:, 0], c[:, 1], c[:, 2], lab, as_tensor=True)
        with path.open("wb") as fh:
            fh.write(b"x,y,z,label\n")
            text.write_text(fh, rows)
        return
    arr = np.column_stack((coords, labels))
    np.savetxt(path, arr, fmt="%.6f,%.6f,%.6f,%d", header="x,y,z,label", comments="")


def save_tracking_results(objects, cluster_rows, output_dir: Path) -> None:
    """PointCloudWork/4_temporal_object_tracker.py:832-886: tracked_objects.csv, trajectories.csv
    and clusters.csv written by pandas from the same Python scalars the reference puts in its
    rows (np.float32 centroids, the exact type of average_velocity, Python float mean
    intensities), so pandas infers the same column dtypes and the files are byte-identical.

    objects: TrackedObject snapshots in tracker dict order (rpt.native_tracker);
    cluster_rows: (frame_id, cluster_id, num_points, cx np.float32, cy np.float32, mean_i float)
    in clusters_by_frame order (frames with clusters, each frame's clusters in reference order).
    """
    import pandas as pd

    output_dir = Path(output_dir)
    output_dir.mkdir(parents=True, exist_ok=True)
    summary = []
    for o in objects:
        seen = o.frames_seen
        summary.append({"object_id": o.object_id, "object_type": o.object_type,
                        "num_frames_seen": len(seen),
                        "first_frame": min(seen) if seen else -1,
                        "last_frame": max(seen) if seen else -1,
                        "avg_velocity": o.average_velocity,
                        "final_x": o.centroid[0], "final_y": o.centroid[1]})
    path = output_dir / "tracked_objects.csv"
    pd.DataFrame(summary).to_csv(path, index=False)
    print(f"Saved object summary to {path}")

    traj = [{"object_id": o.object_id, "object_type": o.object_type, "frame_id": f,
             "x": pos[0], "y": pos[1]}
            for o in objects for pos, f in zip(o.positions, o.frames_seen)]
    path = output_dir / "trajectories.csv"
    pd.DataFrame(traj).to_csv(path, index=False)
    print(f"Saved trajectories to {path}")

    rows = [{"frame_id": fid, "cluster_id": cid, "num_points": n, "centroid_x": cx,
             "centroid_y": cy, "mean_intensity": mi}
            for fid, cid, n, cx, cy, mi in cluster_rows]
    path = output_dir / "clusters.csv"
    pd.DataFrame(rows).to_csv(path, index=False)
    print(f"Saved clusters to {path}")
