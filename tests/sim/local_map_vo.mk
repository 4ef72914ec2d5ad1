# tests/sim/local_map_vo.mk -- TEST AID built by tests/test_local_map_host.py and tests/test_run_vo_local_map_sim.py into
# tests/sim/_build/ (never part of libmvo_hip.so): libmvo_sim_local_map_vo.so = the objects of libmvo_sim_pose_optimize.so
# (pose_optimize.mk: everything run_vo calls) plus csrc/local_map_host.cpp and csrc/local_map_kernels.hip, the two sources of
# local_map.mk, for the programs that run the second search behind the pose optimisation.
#   make -C tests/sim -f local_map_vo.mk _build/libmvo_sim_local_map_vo.so
include pose_optimize.mk
LOCAL_MAP_VO_OBJ := $(POSE_OPTIMIZE_OBJ) _build/full/local_map_host.cpp.o _build/full/local_map_kernels.hip.o
_build/libmvo_sim_local_map_vo.so: $(LOCAL_MAP_VO_OBJ)
	$(CXX) -shared -fPIC -pthread -o $@ $^
