"""Drop-in for the ``radar-pipeline`` click group (radar-pipeline/src/radar_pipeline/cli/main.py:
17-161, 188-253): the same group options (-c/--config YAML, -v, --version) and the same arguments
for ``sort-by-gain``, ``filter-range``, ``convert``, ``build`` and ``cluster`` -- a raw capture
directory to gain folders to Cartesian CSVs, sweep CSVs to stacked PLYs to ST-DBSCAN labels, with
the points, the clustering and the text of the CSV, PLY and label files made on the MI355X.
``visualize`` and the --plot PNGs are outside this engine's scope."""
from __future__ import annotations

import sys
from pathlib import Path
from typing import Optional

import click

from .. import __version__
from ..config import PipelineConfig


@click.group()
@click.option("-c", "--config", type=click.Path(exists=True, path_type=Path),
              help="Path to YAML config file.")
@click.option("-v", "--verbose", count=True, help="Increase verbosity.")
@click.version_option(version=__version__)
@click.pass_context
def cli(ctx: click.Context, config: Optional[Path], verbose: int) -> None:
    """Radar point cloud processing pipeline."""
    ctx.ensure_object(dict)
    ctx.obj["config"] = PipelineConfig.from_yaml(config) if config else PipelineConfig()
    ctx.obj["verbose"] = verbose


@cli.command("sort-by-gain")
@click.argument("directory", type=click.Path(exists=True, path_type=Path))
@click.option("--dry-run", is_flag=True, help="Show what would be moved without moving.")
@click.pass_context
def sort_by_gain(ctx: click.Context, directory: Path, dry_run: bool) -> None:
    """Sort CSV files into gain_40/50/75 folders."""
    from ..processors.sorting import move_files_to_gain_folders

    config: PipelineConfig = ctx.obj["config"]
    moved = move_files_to_gain_folders(directory, config.gains.values, dry_run=dry_run)
    total = sum(len(v) for v in moved.values())
    click.echo(f"{'Would move' if dry_run else 'Moved'} {total} files total.")


@cli.command("filter-range")
@click.argument("directory", type=click.Path(exists=True, path_type=Path))
@click.option("--ranges", "-r", multiple=True, type=int, default=[1, 2],
              help="Range values to remove.")
@click.option("--dry-run", is_flag=True, help="Show what would be deleted without deleting.")
@click.pass_context
def filter_range(ctx: click.Context, directory: Path, ranges: tuple, dry_run: bool) -> None:
    """Remove CSV files with specified Range values."""
    from ..processors.filtering import remove_files_by_range

    config: PipelineConfig = ctx.obj["config"]
    removed = remove_files_by_range(directory, set(ranges), config.gains.values, dry_run=dry_run)
    click.echo(f"{'Would remove' if dry_run else 'Removed'} {len(removed)} files.")


@cli.command("convert")
@click.argument("input_path", type=click.Path(exists=True, path_type=Path))
@click.argument("output_path", type=click.Path(path_type=Path))
@click.option("--threshold", "-t", type=float, default=0.0, help="Intensity threshold.")
@click.option("--batch/--single", default=False, help="Batch mode for aligned gains.")
@click.option("--limit", type=int, help="Limit number of files in batch mode.")
@click.pass_context
def convert(ctx: click.Context, input_path: Path, output_path: Path, threshold: float,
            batch: bool, limit: Optional[int]) -> None:
    """Convert radar CSV to Cartesian coordinates."""
    from ..processors.cartesian import convert_batch_aligned, convert_single_csv

    config: PipelineConfig = ctx.obj["config"]
    # as the reference: neither mode hands the YAML's radar section on (default RadarConfig)
    if batch:
        convert_batch_aligned(input_path, output_path, config.gains.values, threshold, limit)
        click.echo("Batch conversion complete.")
    else:
        n_points = convert_single_csv(input_path, output_path, threshold)
        click.echo(f"Saved {n_points:,} points to {output_path}")


@cli.command("build")
@click.argument("input_dir", type=click.Path(exists=True, path_type=Path))
@click.argument("output_dir", type=click.Path(path_type=Path))
@click.option("--flat/--no-flat", default=True, help="Generate flat stack.")
@click.option("--offset/--no-offset", default=True, help="Generate offset stack.")
@click.option("--plot/--no-plot", default=True, help="Generate PNG previews.")
@click.pass_context
def build(ctx: click.Context, input_dir: Path, output_dir: Path, flat: bool, offset: bool,
          plot: bool) -> None:
    """Build stacked PLY point clouds from Cartesian CSVs."""
    from ..processors.point_cloud import build_stacked_clouds

    config: PipelineConfig = ctx.obj["config"]
    build_stacked_clouds(input_dir, output_dir, config.processing, config.gains, config.radar,
                         generate_flat=flat, generate_offset=offset)
    if plot:
        click.echo("note: the --plot PNG is not rendered by rpt", err=True)
    click.echo("Build complete.")


@cli.command("cluster")
@click.argument("ply_file", type=click.Path(exists=True, path_type=Path))
@click.option("--output-dir", "-o", type=click.Path(path_type=Path), help="Output directory.")
@click.option("--eps-space", type=float, help="Spatial epsilon.")
@click.option("--eps-time", type=float, help="Temporal epsilon.")
@click.option("--min-samples", type=int, help="Minimum samples per cluster.")
@click.option("--max-points", type=int, help="Maximum points to process.")
@click.option("--plot/--no-plot", default=True, help="Generate PNG visualization.")
@click.pass_context
def cluster(ctx: click.Context, ply_file: Path, output_dir: Optional[Path],
            eps_space: Optional[float], eps_time: Optional[float], min_samples: Optional[int],
            max_points: Optional[int], plot: bool) -> None:
    """Run ST-DBSCAN clustering on point cloud."""
    from ..processors.clustering import process_ply_clustering

    config: PipelineConfig = ctx.obj["config"]
    cc = config.clustering.model_copy()
    for name, val in (("eps_space", eps_space), ("eps_time", eps_time),
                      ("min_samples", min_samples), ("max_points", max_points)):
        if val is not None:
            setattr(cc, name, val)
    if output_dir is None:
        output_dir = ply_file.parent
    csv_path, _ = process_ply_clustering(ply_file, output_dir, cc, config.gains)
    if plot:
        click.echo("note: the --plot PNG is not rendered by rpt", err=True)
    click.echo(f"Clustering complete. Labels saved to {csv_path}")


if __name__ == "__main__":
    cli(sys.argv[1:])
