# Top-level build: libc2d.so (HIP, gfx950 only), the CPU oracle, and the CLI drivers.
PKG      := convex-2d-gpu-collision-detection_amd
CSRC     := $(PKG)/csrc
LIBDIR   := $(PKG)/lib
HIPCC    ?= /opt/rocm/bin/hipcc
# -ffp-contract=off is part of the arithmetic contract: no implicit FMA.
# -fno-slp-vectorize: hipcc otherwise packs scalar f32 ops into v_pk_mul/add_f32, measured 2 % slower here.
HIPFLAGS := -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -fno-slp-vectorize -fPIC -Wall -Wextra -Wno-unused-parameter -Iinclude

SRCS := $(CSRC)/c2d_api.hip $(CSRC)/c2d_host.hip $(CSRC)/c2d_sat.hip $(CSRC)/c2d_poly.hip $(CSRC)/c2d_poly_binned.hip $(CSRC)/c2d_mc.hip $(CSRC)/c2d_mc_poly.hip $(CSRC)/c2d_tables.hip $(CSRC)/c2d_dist.hip $(CSRC)/c2d_cross.hip $(CSRC)/c2d_broad.hip $(CSRC)/c2d_poly_cross.hip $(CSRC)/c2d_poly_broad.hip $(CSRC)/c2d_contact.hip $(CSRC)/c2d_distance.hip $(CSRC)/c2d_overlap.hip $(CSRC)/c2d_ray.hip $(CSRC)/c2d_ray_grid.hip $(CSRC)/c2d_sweep.hip $(CSRC)/c2d_clearance.hip $(CSRC)/c2d_cast.hip $(CSRC)/c2d_sweep_broad.hip $(CSRC)/c2d_near_broad.hip $(CSRC)/c2d_clearance_grid.hip $(CSRC)/c2d_cast_grid.hip
OBJS := $(SRCS:.hip=.o)
HDRS := $(CSRC)/c2d_math.hpp $(CSRC)/c2d_mc_core.hpp $(CSRC)/c2d_count.hpp $(CSRC)/c2d_internal.hpp $(CSRC)/c2d_broad.hpp $(CSRC)/c2d_poly_pair.hpp $(CSRC)/c2d_poly_broad_box.hpp $(CSRC)/c2d_cross.hpp $(CSRC)/c2d_cross_tiles.hpp $(CSRC)/c2d_pair_list.hpp $(CSRC)/c2d_ray_strips.hpp $(CSRC)/c2d_ray_rule.hpp $(CSRC)/c2d_ray_walk.hpp $(CSRC)/c2d_distance_rule.hpp $(CSRC)/c2d_overlap_rule.hpp $(CSRC)/c2d_clearance_bound.hpp $(CSRC)/c2d_clearance_parts.hpp $(CSRC)/c2d_near_shape.hpp $(CSRC)/c2d_sweep_rule.hpp $(CSRC)/c2d_sweep_shape.hpp $(CSRC)/c2d_cast_parts.hpp $(CSRC)/c2d_grid_best.hpp $(CSRC)/c2d_set_best.hpp $(CSRC)/c2d_wave.hpp include/c2d.h include/utils.h

all: lib oracle drivers lib-fmad lib-nopretest lib-rehearsal lib-movecheck lib-splitcheck

lib: $(LIBDIR)/libc2d.so

$(CSRC)/%.o: $(CSRC)/%.hip $(HDRS)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(LIBDIR)/libc2d.so: $(OBJS)
	@mkdir -p $(LIBDIR)
	$(HIPCC) --offload-arch=gfx950 -shared -fPIC -o $@ $(OBJS) -ldl

oracle:
	$(MAKE) -C oracle

# CLI drivers: plain C++17 against the C-ABI only (no HIP headers needed)
BINDIR := $(PKG)/bin
HOST   := $(CSRC)/host
CXX    ?= g++
drivers: $(BINDIR)/generate_dataset $(BINDIR)/compute_collision_probability $(BINDIR)/ztest
$(BINDIR)/%: $(HOST)/%.cpp $(HOST)/driver_common.hpp $(HOST)/npy.hpp $(HOST)/cli.hpp include/c2d.h include/utils.h $(LIBDIR)/libc2d.so
	@mkdir -p $(BINDIR)
	$(CXX) -O2 -std=c++17 -pthread -Wall -Wextra $< -o $@ -L$(LIBDIR) -lc2d -Wl,-rpath,'$$ORIGIN/../lib' -Wl,-rpath-link,/opt/rocm/lib

clean:
	rm -f $(OBJS) $(LIBDIR)/libc2d.so $(BINDIR)/generate_dataset $(BINDIR)/compute_collision_probability $(BINDIR)/ztest
	$(MAKE) -C oracle clean

.PHONY: all lib oracle drivers tools clean lib-fmad lib-nopretest lib-rehearsal lib-mcstats lib-mcclock lib-ab-stamps lib-ab-clearance lib-movecheck lib-splitcheck

# developer tools (not shipped in libc2d.so)
TOOLS := $(CSRC)/tools/sat_tune $(CSRC)/tools/pose_probe $(CSRC)/tools/clock_probe $(CSRC)/tools/instr_probe $(CSRC)/tools/store_pattern_probe $(CSRC)/tools/stream_lifetime_probe $(CSRC)/tools/load_policy_probe
tools: $(TOOLS)
# (the instruction probe includes the Monte-Carlo legs' mixes when profiles/valu_issue.py has generated them)
$(CSRC)/tools/instr_probe: $(wildcard $(CSRC)/tools/instr_probe_mixes.inc)
$(CSRC)/tools/%: $(CSRC)/tools/%.hip $(HDRS)
	$(HIPCC) -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -fno-slp-vectorize -Iinclude $< -o $@

# validation build: Monte-Carlo kernels without the certain-miss pretests (tests/test_gpu_fullsize.py, tools/validate_*.py)
lib-nopretest: $(LIBDIR)/libc2d_nopretest.so
$(CSRC)/c2d_mc_nopretest.o: $(CSRC)/c2d_mc.hip $(HDRS)
	$(HIPCC) $(HIPFLAGS) -DC2D_MC_NO_PRETEST -DC2D_MC_NO_AXIS_SKIP -DC2D_MC_NO_MODEL_TEST -c $< -o $@
$(LIBDIR)/libc2d_nopretest.so: $(OBJS) $(CSRC)/c2d_mc_nopretest.o
	$(HIPCC) --offload-arch=gfx950 -shared -fPIC -o $@ $(filter-out $(CSRC)/c2d_mc.o,$(OBJS)) $(CSRC)/c2d_mc_nopretest.o -ldl

# validation builds: the reference's dot products contracted as nvcc -fmad=true might (C2D_FMAD in c2d_math.hpp);
# only used to measure the distance from the canonical arithmetic (tests/test_gpu_fmad.py)
lib-fmad: $(LIBDIR)/libc2d_fmad1.so $(LIBDIR)/libc2d_fmad2.so
$(LIBDIR)/libc2d_fmad%.so: $(SRCS) $(HDRS)
	@mkdir -p $(LIBDIR) build/fmad$*
	for f in $(SRCS); do $(HIPCC) $(HIPFLAGS) -DC2D_FMAD=$* -c $$f -o build/fmad$*/$$(basename $$f .hip).o || exit 1; done
	$(HIPCC) --offload-arch=gfx950 -shared -fPIC -o $@ build/fmad$*/*.o -ldl

# rehearsal build (tests only): the same library with c2d_dist's file transport compiled in, under the product's file
# name in its own directory, so that LD_LIBRARY_PATH / C2D_LIBRARY can put it in front of the product library for the
# two-ranks-on-one-GPU tests (tests/test_gpu_dist.py).  The product libc2d.so contains no such transport.
REHDIR := $(PKG)/lib-rehearsal
lib-rehearsal: $(REHDIR)/libc2d.so
$(CSRC)/c2d_dist_rehearsal.o: $(CSRC)/c2d_dist.hip $(HDRS)
	$(HIPCC) $(HIPFLAGS) -DC2D_DIST_REHEARSAL -c $< -o $@
$(REHDIR)/libc2d.so: $(OBJS) $(CSRC)/c2d_dist_rehearsal.o
	@mkdir -p $(REHDIR)
	$(HIPCC) --offload-arch=gfx950 -shared -fPIC -o $@ $(filter-out $(CSRC)/c2d_dist.o,$(OBJS)) $(CSRC)/c2d_dist_rehearsal.o -ldl

# developer build: the binning pass's move kernel checks every index against its array and reports the first offender on
# stderr instead of making the access (C2D_MOVE_CHECK in c2d_poly_binned.hip); run anything on it with C2D_LIBRARY=...
lib-movecheck: $(LIBDIR)/libc2d_movecheck.so
$(CSRC)/c2d_poly_binned_movecheck.o: $(CSRC)/c2d_poly_binned.hip $(HDRS)
	$(HIPCC) $(HIPFLAGS) -DC2D_MOVE_CHECK -c $< -o $@
$(LIBDIR)/libc2d_movecheck.so: $(OBJS) $(CSRC)/c2d_poly_binned_movecheck.o
	@mkdir -p $(LIBDIR)
	$(HIPCC) --offload-arch=gfx950 -shared -fPIC -o $@ $(filter-out $(CSRC)/c2d_poly_binned.o,$(OBJS)) $(CSRC)/c2d_poly_binned_movecheck.o -ldl

# test build: the index-checked binning pass with a plane limit of 32 KiB instead of 4 GiB (C2D_FROM_PADDED_PLANE_MAX), so that
# c2d_poly_bins_from_padded splits classes of a few hundred to a few thousand pairs into several bins (tests/test_gpu_poly_binned.py)
lib-splitcheck: $(LIBDIR)/libc2d_splitcheck.so
$(CSRC)/c2d_poly_binned_splitcheck.o: $(CSRC)/c2d_poly_binned.hip $(HDRS)
	$(HIPCC) $(HIPFLAGS) -DC2D_MOVE_CHECK -DC2D_FROM_PADDED_PLANE_MAX=32768 -c $< -o $@
$(LIBDIR)/libc2d_splitcheck.so: $(OBJS) $(CSRC)/c2d_poly_binned_splitcheck.o
	@mkdir -p $(LIBDIR)
	$(HIPCC) --offload-arch=gfx950 -shared -fPIC -o $@ $(filter-out $(CSRC)/c2d_poly_binned.o,$(OBJS)) $(CSRC)/c2d_poly_binned_splitcheck.o -ldl

# census build (developer tool, not part of `all`): Monte-Carlo kernels that count where their samples go (C2D_MC_STATS in c2d_mc.hip);
# tests/tools/mc_stats.py reads the counters and records the evaluated-sample fraction the bench quotes
lib-mcstats: $(LIBDIR)/libc2d_mcstats.so
$(CSRC)/c2d_mc_stats.o: $(CSRC)/c2d_mc.hip $(HDRS)
	$(HIPCC) $(HIPFLAGS) -DC2D_MC_STATS -c $< -o $@
$(CSRC)/c2d_mc_poly_stats.o: $(CSRC)/c2d_mc_poly.hip $(HDRS)
	$(HIPCC) $(HIPFLAGS) -DC2D_MC_STATS -c $< -o $@
$(LIBDIR)/libc2d_mcstats.so: $(OBJS) $(CSRC)/c2d_mc_stats.o $(CSRC)/c2d_mc_poly_stats.o
	$(HIPCC) --offload-arch=gfx950 -shared -fPIC -o $@ $(filter-out $(CSRC)/c2d_mc.o $(CSRC)/c2d_mc_poly.o,$(OBJS)) $(CSRC)/c2d_mc_stats.o $(CSRC)/c2d_mc_poly_stats.o -ldl

# clock build (developer tool, not part of `all`): Monte-Carlo kernels that stamp s_memtime / s_memrealtime around their sample work
# (C2D_MC_CLOCK in c2d_mc_core.hpp); tests/tools/mc_clock.py reads the stamps and records the clock the kernels hold
lib-mcclock: $(LIBDIR)/libc2d_mcclock.so
$(CSRC)/c2d_mc_clock.o: $(CSRC)/c2d_mc.hip $(HDRS)
	$(HIPCC) $(HIPFLAGS) -DC2D_MC_CLOCK -c $< -o $@
$(CSRC)/c2d_mc_poly_clock.o: $(CSRC)/c2d_mc_poly.hip $(HDRS)
	$(HIPCC) $(HIPFLAGS) -DC2D_MC_CLOCK -c $< -o $@
$(LIBDIR)/libc2d_mcclock.so: $(OBJS) $(CSRC)/c2d_mc_clock.o $(CSRC)/c2d_mc_poly_clock.o
	$(HIPCC) --offload-arch=gfx950 -shared -fPIC -o $@ $(filter-out $(CSRC)/c2d_mc.o $(CSRC)/c2d_mc_poly.o,$(OBJS)) $(CSRC)/c2d_mc_clock.o $(CSRC)/c2d_mc_poly_clock.o -ldl

# measurement builds (developer tool, not part of `all`): what the completion stamps of the workspace guard cost the counting kernels
# (csrc/c2d_count.hpp C2D_WS_STAMP_MODE: 0 = none, 2 = with a release fence; the product is 1); compared with the product library in one
# process by csrc/tools/rect_bench.py (profiles/notes_r05_workspace_guard.md)
lib-ab-stamps: $(LIBDIR)/libc2d_stamp0.so $(LIBDIR)/libc2d_stamp2.so
$(LIBDIR)/libc2d_stamp%.so: $(SRCS) $(HDRS)
	@mkdir -p $(LIBDIR) build/stamp$*
	for f in $(SRCS); do $(HIPCC) $(HIPFLAGS) -DC2D_WS_STAMP_MODE=$* -c $$f -o build/stamp$*/$$(basename $$f .hip).o || exit 1; done
	$(HIPCC) --offload-arch=gfx950 -shared -fPIC -o $@ build/stamp$*/*.o -ldl

# measurement build (developer tool, not part of `all`): the clearance kernel without its certified skip (C2D_CLEARANCE_NO_SKIP in
# c2d_clearance.hip), compared with the product library in one process by csrc/tools/clearance_bench.py (profiles/notes_r18_clearances.md)
lib-ab-clearance: $(LIBDIR)/libc2d_clr_noskip.so
$(CSRC)/c2d_clearance_noskip.o: $(CSRC)/c2d_clearance.hip $(HDRS)
	$(HIPCC) $(HIPFLAGS) -DC2D_CLEARANCE_NO_SKIP -c $< -o $@
$(LIBDIR)/libc2d_clr_noskip.so: $(OBJS) $(CSRC)/c2d_clearance_noskip.o
	$(HIPCC) --offload-arch=gfx950 -shared -fPIC -o $@ $(filter-out $(CSRC)/c2d_clearance.o,$(OBJS)) $(CSRC)/c2d_clearance_noskip.o -ldl
