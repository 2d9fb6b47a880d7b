"""Drop-in for ``radar_pipeline.processors.filtering`` (radar-pipeline/src/radar_pipeline/
processors/filtering.py): CSVs of unwanted Range settings removed from the ``gain_{g}`` folders.
Host-only file management."""
from __future__ import annotations

from pathlib import Path
from typing import Iterator, List, Optional, Set, Tuple

from ..config import GainConfig
from .sorting import _first_row_int


def get_csv_range(path: Path) -> Optional[int]:
    """filtering.py:12-40: the Range column (third field) of the first data row."""
    return _first_row_int(path, 2)


def find_targets(base_dir: Path, gains: Optional[Tuple[int, ...]] = None) -> Iterator[Path]:
    """filtering.py:43-69: the ``*.csv`` of every existing ``base_dir/gain_{g}`` in directory
    order (not sorted)."""
    if gains is None:
        gains = GainConfig().values
    for g in gains:
        folder = Path(base_dir) / f"gain_{g}"
        if folder.is_dir():
            yield from folder.glob("*.csv")


def find_files_by_range(base_dir: Path, ranges_to_find: Set[int],
                        gains: Optional[Tuple[int, ...]] = None) -> List[Path]:
    """filtering.py:72-99"""
    return [p for p in find_targets(base_dir, gains) if get_csv_range(p) in ranges_to_find]


def remove_files_by_range(base_dir: Path, ranges_to_remove: Set[int],
                          gains: Optional[Tuple[int, ...]] = None,
                          dry_run: bool = False) -> List[Path]:
    """filtering.py:102-141: the matching files listed on stdout and, unless dry_run, deleted."""
    doomed = find_files_by_range(base_dir, ranges_to_remove, gains)
    if not doomed:
        print(f"No files with Range in {ranges_to_remove} found.")
        return []
    print(f"{'Would delete' if dry_run else 'Deleting'} {len(doomed)} files:")
    for path in doomed:
        print(f"  - {path}")
        if not dry_run:
            path.unlink(missing_ok=True)
    return doomed
