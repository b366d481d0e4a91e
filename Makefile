# Builds the product library (HIP, gfx950 only) and the CPU oracle (test infrastructure).
HIPCC   ?= hipcc
ARCH    ?= gfx950
CSRC    := fsae-mpc_amd/csrc
LIBDIR  := fsae-mpc_amd/lib
HIPFLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -Iinclude -I$(CSRC) -Wall -Wno-unused-function

all: $(LIBDIR)/libfsaempc.so oracle o1 dbg

# Every device translation unit is compiled through tools/hipcc_checked.sh: device code via assembly text, which is checked (and,
# if need be, repaired) for the compiler defect of DESIGN.md "Build-variant fragility: root cause" before it is assembled; the
# report of each unit stays next to its object (*.isa.log; `make isa-report` prints them).
CC_CHECKED := HIPCC=$(HIPCC) tools/hipcc_checked.sh
CHECKDEPS := tools/hipcc_checked.sh tools/check_isa_exec_prologue.py

$(LIBDIR)/%.o: $(CSRC)/%.hip $(CSRC)/qp_solver.h $(CSRC)/qp_sens.h $(CSRC)/ltv_build.h $(CSRC)/nlp_model.h $(CSRC)/ltv_model.h $(CSRC)/mpc_params.h $(CSRC)/sqp.h $(CSRC)/reference.h $(CSRC)/plant.h $(CSRC)/planner.h $(CSRC)/raceline.h $(CSRC)/corridor.h $(CSRC)/cones.h $(CSRC)/cl_frame.h include/fsaempc.h $(CHECKDEPS)
	@mkdir -p $(LIBDIR)
	$(CC_CHECKED) $@ $< $(HIPFLAGS)

# the C ABI (host-side glue, one unit per subsystem, built by the rule above): what the units share is read by them only
CAPIOBJ := $(LIBDIR)/capi_qp.o $(LIBDIR)/capi_ltv.o $(LIBDIR)/capi_cl.o $(LIBDIR)/capi_plan.o
$(CAPIOBJ): $(CSRC)/capi_common.h

# the body of the LTV build kernel: read by the two units that instantiate it, without and with blocks
$(LIBDIR)/ltv_build.o $(LIBDIR)/ltv_build_blocked.o: $(CSRC)/ltv_build_kernel.h

# the minimum-time line: its own header, read by its unit and the C ABI's planning unit only
$(LIBDIR)/minlap.o $(LIBDIR)/capi_plan.o: $(CSRC)/minlap.h

# the speed profile of the plans: its rules and kernel phases, read by the three plan units (and through minlap.h by
# the C ABI's planning unit); the body of the plan kernel, read by the two units that instantiate it, on the centre line and on a line
$(LIBDIR)/planner.o $(LIBDIR)/raceline.o $(LIBDIR)/minlap.o $(LIBDIR)/capi_plan.o: $(CSRC)/plan_profile.h
$(LIBDIR)/planner.o $(LIBDIR)/raceline.o: $(CSRC)/plan_profile_kernel.h

# measurement noise, plan latency and delay compensation of the closed loop: likewise, the C ABI's closed-loop unit
$(LIBDIR)/cl_latency.o $(LIBDIR)/capi_cl.o: $(CSRC)/cl_latency.h

# the state estimator of the closed loop: likewise
$(LIBDIR)/cl_estimator.o $(LIBDIR)/capi_cl.o: $(CSRC)/cl_estimator.h

# the Cartesian sensor models of the closed loop: likewise; their unit reads the rules of the two units above too
$(LIBDIR)/cl_sensors.o $(LIBDIR)/capi_cl.o: $(CSRC)/cl_sensors.h
$(LIBDIR)/cl_sensors.o: $(CSRC)/cl_latency.h $(CSRC)/cl_estimator.h

# cone-based localisation: the cone sensor's unit; the filter with the cone rows lives in the unit of the Cartesian filter
$(LIBDIR)/cl_cone_loc.o $(LIBDIR)/cl_sensors.o $(LIBDIR)/capi_cl.o: $(CSRC)/cl_cone_loc.h
$(LIBDIR)/cl_cone_loc.o: $(CSRC)/cl_latency.h $(CSRC)/cl_sensors.h $(CSRC)/qp_lane.h

# the SQP as the controller of the closed loop: likewise, and the SQP's host loop (its skip mask)
$(LIBDIR)/cl_nmpc.o $(LIBDIR)/capi_cl.o $(LIBDIR)/capi_ltv.o: $(CSRC)/cl_nmpc.h

# WGFLAGS (both solve kernels): without machine LICM and with sinking-to-avoid-spills the T = 8 workgroup kernel spills 20 VGPRs
# instead of 166 (256 are its budget at two waves per SIMD) and the one-wavefront kernels need no scratch at all (T = 5: 140..504
# bytes per lane before): hoisted address arithmetic no longer lives across the whole iteration loop.
WGFLAGS := -mllvm -disable-machine-licm -mllvm -sink-insts-to-avoid-spills=1

# (qp_rules.h: the scalar rules of the algorithm, read by both solve kernels -- every solver unit and variant depends on it)
# qp_solver.hip is compiled as five translation units (see the note in the file): main + the tile counts T = 1..4, 5, 6, 7
QPHDRS := $(CSRC)/qp_solver.h $(CSRC)/qp_lane.h $(CSRC)/qp_rules.h $(CSRC)/qp_solve_kernel.h $(CSRC)/qp_selftest.h $(CSRC)/qp_probe.h
WGHDRS := $(CSRC)/qp_solver.h $(CSRC)/qp_lane.h $(CSRC)/qp_rules.h
QPOBJ := $(LIBDIR)/qp_solver_tu0.o $(LIBDIR)/qp_solver_tu1.o $(LIBDIR)/qp_solver_tu2.o $(LIBDIR)/qp_solver_tu3.o $(LIBDIR)/qp_solver_tu4.o
$(LIBDIR)/qp_solver_tu%.o: $(CSRC)/qp_solver.hip $(QPHDRS) include/fsaempc.h $(CHECKDEPS)
	@mkdir -p $(LIBDIR)
	$(CC_CHECKED) $@ $< $(HIPFLAGS) $(WGFLAGS) -DQP_TU=$*

# qp_wg.hip (workgroup-per-QP solve kernel, tile counts T = 1..12) is compiled once per range of tile counts (lo_hi)
WGOBJ := $(LIBDIR)/qp_wg_1_5.o $(LIBDIR)/qp_wg_6_6.o $(LIBDIR)/qp_wg_7_7.o $(LIBDIR)/qp_wg_8_8.o $(LIBDIR)/qp_wg_9_9.o $(LIBDIR)/qp_wg_10_10.o $(LIBDIR)/qp_wg_11_11.o $(LIBDIR)/qp_wg_12_12.o
$(LIBDIR)/qp_wg_%.o: $(CSRC)/qp_wg.hip $(WGHDRS) include/fsaempc.h $(CHECKDEPS)
	@mkdir -p $(LIBDIR)
	$(CC_CHECKED) $@ $< $(HIPFLAGS) $(WGFLAGS) -DQP_WG_TLO=$(word 1,$(subst _, ,$*)) -DQP_WG_THI=$(word 2,$(subst _, ,$*))

# host-side track pipeline (no device code)
$(LIBDIR)/track.o: $(CSRC)/track.cpp include/fsaempc.h
	@mkdir -p $(LIBDIR)
	g++ -O2 -std=c++17 -fPIC -Wall -Iinclude -c $< -o $@

COMMON := $(LIBDIR)/ltv_build.o $(LIBDIR)/ltv_build_blocked.o $(LIBDIR)/sqp.o $(LIBDIR)/qp_sens.o $(LIBDIR)/reference.o $(LIBDIR)/plant.o $(LIBDIR)/cl_latency.o $(LIBDIR)/cl_estimator.o $(LIBDIR)/cl_sensors.o $(LIBDIR)/cl_cone_loc.o $(LIBDIR)/cl_nmpc.o $(LIBDIR)/planner.o $(LIBDIR)/raceline.o $(LIBDIR)/minlap.o $(LIBDIR)/corridor.o $(LIBDIR)/cones.o $(CAPIOBJ) $(LIBDIR)/track.o
$(LIBDIR)/libfsaempc.so: $(QPOBJ) $(WGOBJ) $(COMMON)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $^

# development: qp_solver.hip as ONE unit for a single tile count (EXP_T) with extra flags (EXP_FLAGS: -DQP_STAMPS=1, -DQP_PROBE, ...)
# through the checked pipeline, linked with the shipped objects of everything else -> libfsaempc_$(EXP_NAME).so (FSAEMPC_LIB selects
# it).  tools/build_exp.sh is the front end.  Always rebuilt: the flags are not part of the target's name.
EXP_T ?= 5
EXP_FLAGS ?=
EXP_NAME ?= exp
exp: $(WGOBJ) $(COMMON)
	$(CC_CHECKED) $(LIBDIR)/$(EXP_NAME)_qp_solver.o $(CSRC)/qp_solver.hip $(filter-out -Wall,$(HIPFLAGS)) -DQP_ONLY_T=$(EXP_T) $(EXP_FLAGS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $(LIBDIR)/libfsaempc_$(EXP_NAME).so $(LIBDIR)/$(EXP_NAME)_qp_solver.o $(WGOBJ) $(COMMON)

# development builds of the workgroup kernel: ONE instantiation (T = 8 + slack border: BASELINE configs[2], dynamic N = 60) linked with the
# shipped objects of everything else; plain and with phase stamps.  Select with FSAEMPC_LIB.
WGDEVFLAGS := $(WGFLAGS) -DQP_WG_TLO=8 -DQP_WG_THI=8 -DQP_WG_ONLY_NB=4
$(LIBDIR)/wgdev_qp_wg.o: $(CSRC)/qp_wg.hip $(WGHDRS) include/fsaempc.h
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) $(WGDEVFLAGS) -c $< -o $@
$(LIBDIR)/wgdevst_qp_wg.o: $(CSRC)/qp_wg.hip $(WGHDRS) include/fsaempc.h
	@mkdir -p $(LIBDIR)
	$(HIPCC) $(HIPFLAGS) $(WGDEVFLAGS) -DQP_STAMPS=1 -c $< -o $@
WGDEVREST := $(QPOBJ) $(filter-out $(LIBDIR)/qp_wg_8_8.o,$(WGOBJ)) $(COMMON)
wgdev: $(LIBDIR)/libfsaempc_wgdev.so $(LIBDIR)/libfsaempc_wgdevst.so
$(LIBDIR)/libfsaempc_wgdev.so: $(LIBDIR)/wgdev_qp_wg.o $(WGDEVREST)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $^
$(LIBDIR)/libfsaempc_wgdevst.so: $(LIBDIR)/wgdevst_qp_wg.o $(WGDEVREST)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $^

# diagnostic library with the in-kernel dump hooks of both kernels (tests/test_gpu_parity.py::test_01_normal_matrix_dump_matches_numpy); T <= 5
DBGOBJ := $(LIBDIR)/dbg_qp_solver_tu0.o $(LIBDIR)/dbg_qp_solver_tu1.o $(LIBDIR)/dbg_qp_solver_tu2.o $(LIBDIR)/dbg_qp_wg_1_5.o
$(LIBDIR)/dbg_qp_wg_%.o: $(CSRC)/qp_wg.hip $(WGHDRS) include/fsaempc.h $(CHECKDEPS)
	@mkdir -p $(LIBDIR)
	$(CC_CHECKED) $@ $< $(HIPFLAGS) $(WGFLAGS) -DQP_DEBUG_DUMP -DQP_WG_TLO=$(word 1,$(subst _, ,$*)) -DQP_WG_THI=$(word 2,$(subst _, ,$*))
$(LIBDIR)/dbg_qp_solver_tu%.o: $(CSRC)/qp_solver.hip $(QPHDRS) include/fsaempc.h $(CHECKDEPS)
	@mkdir -p $(LIBDIR)
	$(CC_CHECKED) $@ $< $(HIPFLAGS) $(WGFLAGS) -DQP_DEBUG_DUMP -DQP_TU=$*
dbg: $(LIBDIR)/libfsaempc_dbg.so
$(LIBDIR)/libfsaempc_dbg.so: $(DBGOBJ) $(LIBDIR)/qp_solver_tu3.o $(LIBDIR)/qp_solver_tu4.o $(filter-out $(LIBDIR)/qp_wg_1_5.o,$(WGOBJ)) $(COMMON)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $^

# guard build: the solver sources at -O1, every instantiated (T, NB) (tests/test_gpu_parity.py::test_shipped_build_matches_O1_build
# compares the two builds on the GPU; see DESIGN.md "Build-variant fragility")
O1FLAGS := --offload-arch=$(ARCH) -O1 -std=c++17 -fPIC -Iinclude -I$(CSRC) -Wno-unused-function $(WGFLAGS)
O1OBJ := $(LIBDIR)/o1_qp_solver_tu0.o $(LIBDIR)/o1_qp_solver_tu1.o $(LIBDIR)/o1_qp_solver_tu2.o $(LIBDIR)/o1_qp_solver_tu3.o $(LIBDIR)/o1_qp_solver_tu4.o \
         $(LIBDIR)/o1_qp_wg_1_5.o $(LIBDIR)/o1_qp_wg_6_6.o $(LIBDIR)/o1_qp_wg_7_7.o $(LIBDIR)/o1_qp_wg_8_8.o $(LIBDIR)/o1_qp_wg_9_9.o $(LIBDIR)/o1_qp_wg_10_10.o \
         $(LIBDIR)/o1_qp_wg_11_11.o $(LIBDIR)/o1_qp_wg_12_12.o
$(LIBDIR)/o1_qp_solver_tu%.o: $(CSRC)/qp_solver.hip $(QPHDRS) include/fsaempc.h $(CHECKDEPS)
	@mkdir -p $(LIBDIR)
	$(CC_CHECKED) $@ $< $(O1FLAGS) -DQP_TU=$*
# (the guard's workgroup kernels take the unpipelined variant of pass 1, -DQP_WG_NOPIPE: an independent code path for the check,
#  and the -O1 build of the pipelined one walks wrong iterates on kinematic N = 64 -- DESIGN.md 5c, open)
$(LIBDIR)/o1_qp_wg_%.o: $(CSRC)/qp_wg.hip $(WGHDRS) include/fsaempc.h $(CHECKDEPS)
	@mkdir -p $(LIBDIR)
	$(CC_CHECKED) $@ $< $(O1FLAGS) -DQP_WG_NOPIPE -DQP_WG_TLO=$(word 1,$(subst _, ,$*)) -DQP_WG_THI=$(word 2,$(subst _, ,$*))
o1: $(LIBDIR)/libfsaempc_O1.so
$(LIBDIR)/libfsaempc_O1.so: $(O1OBJ) $(COMMON)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $^

isa-report:
	@cat $(LIBDIR)/*.isa.log

oracle:
	$(MAKE) -C oracle

clean:
	rm -rf $(LIBDIR)/*.o $(LIBDIR)/*.so $(LIBDIR)/*.isa.log $(LIBDIR)/*.s
	$(MAKE) -C oracle clean
.PHONY: all oracle clean o1 wgdev dbg isa-report exp
