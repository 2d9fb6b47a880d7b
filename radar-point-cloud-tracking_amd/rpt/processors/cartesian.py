"""Drop-in for ``radar_pipeline.processors.cartesian`` (radar-pipeline/src/radar_pipeline/
processors/cartesian.py): a raw polar sweep CSV -> the Cartesian ``x,y,z`` CSV, one file or the
aligned ``gain_*`` folders of a capture.

The sweep is parsed by the native reader, the thresholded points are made on the device
(rpt_sweep_to_points) and stay there until they are text: the rows ``DataFrame.to_csv`` would
write -- every float32 as its shortest round-trip decimal -- are formed by the device formatter
(rpt.core.text.format_xyz_rows) and only the finished bytes cross to the host, through pinned
buffers into the file.  A sweep with a NaN or inf coordinate (an empty Scale field) is formatted
by the pandas expression itself.
"""
from __future__ import annotations

from itertools import islice
from pathlib import Path
from typing import Dict, Iterator, List, Optional, Tuple

from ..config import GainConfig, RadarConfig
from ..core.loaders import load_radar_csv
from ..core.text import format_xyz_rows, write_text
from ..core.transforms import sweep_points_device


def convert_single_csv(input_path: Path, output_path: Path, threshold: float = 0.0,
                       config: Optional[RadarConfig] = None) -> int:
    """cartesian.py:16-55: the samples with intensity > threshold (strict, compared in float32)
    in row-major order as ``x,y,z`` rows under an ``x,y,z`` header; an all-rejected sweep leaves
    the header alone.  Returns the number of points written."""
    input_path, output_path = Path(input_path), Path(output_path)
    sweep = load_radar_csv(input_path, config)
    x, y, z = sweep_points_device(sweep, threshold)
    text = format_xyz_rows(x, y, z, as_tensor=True)
    output_path.parent.mkdir(parents=True, exist_ok=True)
    with output_path.open("wb") as fh:
        fh.write(b"x,y,z\n")
        write_text(fh, text)
    return int(x.numel())


def aligned_inputs(base_dir: Path, gains: Tuple[int, ...]) -> Iterator[Tuple[int, Dict[int, Path]]]:
    """cartesian.py:58-87: (1-based index, {gain: path}) over the sorted ``gain_{g}/*.csv`` lists,
    up to the shortest of them; FileNotFoundError for a folder without a CSV."""
    base_dir = Path(base_dir)
    lists: Dict[int, List[Path]] = {}
    for g in gains:
        folder = base_dir / f"gain_{g}"
        lists[g] = sorted(folder.glob("*.csv"))
        if not lists[g]:
            raise FileNotFoundError(f"No CSVs found in {folder}")
    for k in range(min(len(v) for v in lists.values())):
        yield k + 1, {g: lists[g][k] for g in gains}


def convert_batch_aligned(base_dir: Path, output_dir: Path,
                          gains: Optional[Tuple[int, ...]] = None, threshold: float = 0.0,
                          limit: Optional[int] = None,
                          config: Optional[RadarConfig] = None) -> None:
    """cartesian.py:90-124: every aligned set (at most ``limit`` of them) converted into
    ``output_dir/gain_{g}/{idx:04d}_gain_{g}_cartesian.csv``, one line printed per file."""
    if gains is None:
        gains = GainConfig().values
    output_dir = Path(output_dir)
    for idx, group in islice(aligned_inputs(base_dir, gains), limit):
        for gain, src in group.items():
            out_path = output_dir / f"gain_{gain}" / f"{idx:04d}_gain_{gain}_cartesian.csv"
            n_points = convert_single_csv(src, out_path, threshold, config)
            print(f"[{idx:04d}] gain {gain}: {src.name} -> {out_path} ({n_points:,} points)")
