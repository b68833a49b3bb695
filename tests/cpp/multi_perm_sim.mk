# tests/cpp/multi_perm_sim.mk — TEST CODE: the one rule of multi_perm_sim, beside tests/cpp/Makefile (which it includes
# for CXX, CSRC, SIM_SAN, SIM_HDRS, MULTI_SRC and sanitizer_probe).
#   multi_perm_sim    csrc/multi.hip and csrc/multi_perm.hip compiled UNCHANGED with the host compiler over simt/, with the
#                     address and undefined-behaviour sanitizers, and driven through mi355_spmv_multi_create_permuted /
#                     _execute / _destroy beside a plain object on Ax[perm]: the program of
#                     tests/test_multi_perm_sim_cpu.py, built on demand by it:
#                         make -C tests/cpp -f multi_perm_sim.mk multi_perm_sim
include Makefile

multi_perm_sim: multi_perm_sim.cpp sim_runtime.hpp $(MULTI_SRC) $(CSRC)/multi_perm.hip $(SIM_HDRS)
	$(CXX) -std=c++17 -O1 -g -fno-omit-frame-pointer $(SIM_SAN) -Isimt -o $@ $<
