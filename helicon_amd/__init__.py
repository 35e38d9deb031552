"""helicon_amd — MI355X-native denovo3D (twist, rise, Csym) sweep behind jianglab/helicon's
Python signatures.  Hand-written gfx950 kernels in ``csrc/``, reached through the C ABI of
``include/helicon_hip.h``; importing this package does not touch the GPU."""
from .grid import (CandidateGrid, build_grid, layer_line_mask, radial_band_mask, set_to_periodic_range,
                   shard_bounds, sweep_axis, zoom_spec, filter_spec, phase_spec)
from .denovo3D import (SweepEngine, SweepResult, apply_helical_symmetry, auto_horizontalize,
                       compute_phase_difference_across_meridian, compute_power_spectra,
                       cosine_similarity, cross_correlation_coefficient, down_scale,
                       estimate_helix_rotation_center_diameter, generate_xyz_projections, is_vertical, low_high_pass_filter,
                       low_high_pass_filter_3d, process_one_task,
                       rotate_shift_image, simulate_helical_projection, sweep, symmetrize_transform_map, threshold_data,
                       transform_image, transform_map)
from ._lib import HeliconHipError
from .solver import lsq_reconstruct, lsq_reconstruct_batch
from .symmetry_search import SymmetrySearch, helical_symmetry_search
from .fsc import (calc_frc_2d, calc_fsc, calc_fsc_batch, calc_fsc_per_shell, frc_score, fsc_resolution, half_map_fsc,
                  half_map_fsc_batch)
# the function true_fsc.true_fsc is not re-exported under its own name: that would hide the module helicon_amd.true_fsc
from .true_fsc import (TrueFSC, adaptive_mask_device, distance_transform_edt_sq, gaussian_filter_device, gaussian_taps, label_components,
                       otsu_from_counts, randomize_phases_lowpass, soft_mask_device)
# the function fft_resample takes the package attribute of its module's name: reach the module's other names with
# ``from helicon_amd.fft_resample import ...`` (the command line is ``python -m helicon_amd.fft_resample``)
from .fft_resample import crop_operator, fft_crop, fft_rescale, fft_resample, resample_operator, rescale_operator
from .structure_factor import (StructureFactorMatcher, calculate_structural_factor, match_structural_factors,
                               set_structural_factors)
# the function local_resolution takes the package attribute of its module's name, as fft_resample does: reach the module's
# other names with ``from helicon_amd.local_resolution import ...`` (the command line is ``python -m helicon_amd.local_resolution``)
from .local_resolution import LocalFSC, local_resolution, resolution_from_curve, taper_profile, window_centres
from .align import AlignContext, align_images, align_images_grid
from .pixel_size import calibrate_pixel_size, fft_resolution_range, nudft2d2, ring_maximum, ring_power_curve

__version__ = "0.1.0"
