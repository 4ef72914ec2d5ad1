# tests/sim/undistort.mk -- TEST AID built by tests/test_undistort_sim.py into tests/sim/_build/ (never part of
# libmvo_hip.so): libmvo_sim_undistort.so = the objects of libmvo_sim_init.so (init_finish.mk: those of libmvo_sim.so plus
# init_host.cpp, which run_vo's start from images needs) plus csrc/undistort_host.cpp and csrc/undistort_kernels.hip,
# compiled for x86 against hip_emu/ by the same pattern rule.
#   make -C tests/sim -f undistort.mk _build/libmvo_sim_undistort.so
include init_finish.mk
UNDISTORT_OBJ := $(INIT_OBJ) _build/full/undistort_host.cpp.o _build/full/undistort_kernels.hip.o
_build/libmvo_sim_undistort.so: $(UNDISTORT_OBJ)
	$(CXX) -shared -fPIC -pthread -o $@ $^
