# tests/sim/epipolar.mk -- TEST AID built by tests/test_epipolar_sim.py into tests/sim/_build/ (never part of
# libmvo_hip.so): libmvo_sim_epipolar.so = the objects of libmvo_sim_undistort.so (undistort.mk) plus
# csrc/epipolar_host.cpp and csrc/epipolar_kernels.hip, compiled for x86 against hip_emu/ by the
# same pattern rule: every lane of k_knn2_epipolar runs as a fiber on the CPU.  Every *.mk here names its objects as its
# predecessor's list plus its own, so a translation unit is listed once.
#   make -C tests/sim -f epipolar.mk _build/libmvo_sim_epipolar.so
include undistort.mk
EPIPOLAR_OBJ := $(UNDISTORT_OBJ) _build/full/epipolar_host.cpp.o _build/full/epipolar_kernels.hip.o
_build/libmvo_sim_epipolar.so: $(EPIPOLAR_OBJ)
	$(CXX) -shared -fPIC -pthread -o $@ $^
