# tests/cpp/coo_sim.mk — TEST CODE: the one rule of coo_sim, beside tests/cpp/Makefile (which it includes for CXX, CSRC,
# SIM_SAN and sanitizer_probe).
#   coo_sim           csrc/coo_csr.hip compiled UNCHANGED with the host compiler over simt/, with the address and
#                     undefined-behaviour sanitizers, and driven through mi355_spmv_coo_to_csr, _coo_to_csr_symmetric and
#                     _csr_transpose, and kernel by kernel: the program of tests/test_coo_sim_cpu.py, built on demand by it:
#                         make -C tests/cpp -f coo_sim.mk coo_sim
include Makefile

coo_sim: coo_sim.cpp sim_runtime.hpp sim_io.hpp simt/hip/hip_runtime.h $(CSRC)/coo_csr.hip $(CSRC)/common.hpp ../../include/mi355_spmv.h
	$(CXX) -std=c++17 -O1 -g -fno-omit-frame-pointer $(SIM_SAN) -Isimt -o $@ $<
