"""Drop-in for ``python PointCloudWork/5_gain_fusion_ply_builder.py`` (main :680-736): the same
sub-commands, options, defaults and stdout lines and the same PLY files, with the points, the
percentile normalisation, the colours and the ``"%.4f"`` text made on the MI355X
(rpt.processors.fusion).

    python -m rpt.cli.gain_fusion individual --data-dir D --output-dir O [--max-frames M]
                                             [--mode absolute|max]
    python -m rpt.cli.gain_fusion stacked    --data-dir D --output-dir O [--max-frames 100]
                                             [--time-spacing 10] [--mode absolute|max]
    python -m rpt.cli.gain_fusion comparison --data-dir D --output-dir O [--frame 0]

The PNG previews of the script (plot_point_cloud / plot_3d_point_cloud) are not built: matplotlib
rendering is outside this engine's scope, and nothing is printed or written in their place.
"""
from __future__ import annotations

import argparse
from pathlib import Path

EPILOG = """
Modes:
  individual  - Create separate PLY for each frame
  stacked     - Create single PLY with all frames stacked in Z
  comparison  - Create separate PLYs for each gain at one frame

Examples:
  python 5_gain_fusion_ply_builder.py individual --data-dir ./data --output-dir ./ply
  python 5_gain_fusion_ply_builder.py stacked --data-dir ./data --output-dir ./ply --max-frames 50
  python 5_gain_fusion_ply_builder.py comparison --data-dir ./data --output-dir ./ply --frame 0
        """


def build_parser() -> argparse.ArgumentParser:
    """The reference's parser (:681-724): same sub-commands, option names, types and defaults; the
    path defaults follow rpt.cli.tracker (data beside this file, output below the working
    directory)."""
    here = Path(__file__).resolve().parent
    default_data = here / "data"
    default_output = Path.cwd() / "gain_fused_ply"
    ap = argparse.ArgumentParser(description="Build gain-fused PLY point clouds",
                                 formatter_class=argparse.RawDescriptionHelpFormatter,
                                 epilog=EPILOG)
    sub = ap.add_subparsers(dest="command", help="Build mode")

    def common(p, out):
        p.add_argument("--data-dir", type=Path, default=default_data)
        p.add_argument("--output-dir", type=Path, default=default_output / out)
        return p

    p_ind = common(sub.add_parser("individual", help="Build individual frame PLYs"), "individual")
    p_ind.add_argument("--max-frames", type=int, default=0)
    p_ind.add_argument("--mode", choices=["absolute", "max"], default="absolute",
                       help="Fusion mode: absolute (keep all), max (max per cell)")

    p_stack = common(sub.add_parser("stacked", help="Build stacked temporal PLY"), "stacked")
    p_stack.add_argument("--max-frames", type=int, default=100)
    p_stack.add_argument("--time-spacing", type=float, default=10.0,
                         help="Z spacing between frames")
    p_stack.add_argument("--mode", choices=["absolute", "max"], default="absolute")

    p_comp = common(sub.add_parser("comparison", help="Build per-gain PLYs for one frame"),
                    "comparison")
    p_comp.add_argument("--frame", type=int, default=0, help="Frame index to analyze")

    for p in (p_ind, p_stack, p_comp):
        p.add_argument("--device", default=None, help="rpt: torch device (default cuda:0)")
    return ap


def main(argv=None) -> None:
    ap = build_parser()
    a = ap.parse_args(argv)
    if a.command is None:
        ap.print_help()
        return
    from ..processors import fusion

    if a.command == "individual":
        fusion.build_individual_frames(a.data_dir, a.output_dir, a.max_frames, a.mode,
                                       device=a.device)
    elif a.command == "stacked":
        fusion.build_stacked_sequence(a.data_dir, a.output_dir, a.max_frames, a.time_spacing,
                                      a.mode, device=a.device)
    else:
        fusion.build_gain_comparison(a.data_dir, a.output_dir, a.frame, device=a.device)


if __name__ == "__main__":
    main()
