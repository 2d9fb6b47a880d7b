"""Drop-in for ``radar_pipeline.processors.sorting`` (radar-pipeline/src/radar_pipeline/
processors/sorting.py): raw capture CSVs sorted into the ``gain_{g}`` folders that
``convert --batch`` reads.  Host-only file management."""
from __future__ import annotations

import csv
from pathlib import Path
from typing import Dict, List, Optional, Tuple

from ..config import GainConfig


def _first_row_int(csv_path: Path, column: int) -> Optional[int]:
    """int(float(field)) of one column of the first data row (the line after the header); None
    when there is no such row, the row is shorter or the field is not a number."""
    with Path(csv_path).open("r", newline="") as fh:
        rows = csv.reader(fh)
        next(rows, None)
        row = next(rows, None)
    if row is None or len(row) <= column:
        return None
    try:
        return int(float(row[column]))
    except ValueError:
        return None


def sniff_gain(csv_path: Path) -> Optional[int]:
    """sorting.py:12-40: the Gain column (fourth field) of the first data row."""
    return _first_row_int(csv_path, 3)


def sort_files_by_gain(source_dir: Path,
                       gains: Optional[Tuple[int, ...]] = None) -> Dict[int, List[Path]]:
    """sorting.py:43-72: {gain: sorted paths} of ``source_dir/*.csv``; files of another gain (or
    none) are left out, nothing is moved."""
    if gains is None:
        gains = GainConfig().values
    by_gain: Dict[int, List[Path]] = {g: [] for g in gains}
    for path in sorted(Path(source_dir).glob("*.csv")):
        gain = sniff_gain(path)
        if gain in by_gain:
            by_gain[gain].append(path)
    return by_gain


def move_files_to_gain_folders(source_dir: Path, gains: Optional[Tuple[int, ...]] = None,
                               dry_run: bool = False) -> Dict[int, List[Path]]:
    """sorting.py:75-125: every ``source_dir/*.csv`` of a known gain renamed into
    ``source_dir/gain_{g}/`` (folders made first), one line printed per file.  dry_run only
    prints.  Returns {gain: new paths} (the untouched source paths on a dry run)."""
    if gains is None:
        gains = GainConfig().values
    source_dir = Path(source_dir)
    moved: Dict[int, List[Path]] = {g: [] for g in gains}
    if not dry_run:
        for g in gains:
            (source_dir / f"gain_{g}").mkdir(parents=True, exist_ok=True)
    for path in sorted(source_dir.glob("*.csv")):
        gain = sniff_gain(path)
        if gain not in moved:
            continue
        folder = f"gain_{gain}"
        if dry_run:
            print(f"Would move gain {gain}: {path.name} -> {folder}/")
            moved[gain].append(path)
        else:
            dest = source_dir / folder / path.name
            path.rename(dest)
            print(f"Moved gain {gain}: {path.name} -> {folder}/")
            moved[gain].append(dest)
    return moved
