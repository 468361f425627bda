#!/bin/bash
# check_switches.sh: the documented S5FXP_* experiment switches (include/s5fxp.h "Environment") must not change results.
# tests/test_variant_matrix.py creates one engine per switch in one process and compares every workload with the CPU oracle;
# tests/test_cpu_suite.py keeps the switch names of the library, the header and the scripts in agreement.
python3 -m pytest tests/test_variant_matrix.py -q -m gpu "$@"
