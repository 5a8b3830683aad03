// Unsteady linear elasticity driver on the MI355X path: the reference's unsteadyLinElas test
// (feddlib/problems/tests/unsteadyLinElas/main.cpp:86-316) written against the FEDD:: operator surface -- same XML parameter
// files, same call sequence
//   BCBuilder::addBC(zero Dirichlet) -> LinElas(...) -> addRhsFunction(rhs2D | rhs) -> addParemeterRhs(force, ramp end, degree)
//   -> addBoundaries -> initializeProblem -> assemble -> DAESolverInTime(parameterListAll, comm) -> defineTimeStepping(1 x 1)
//   -> setProblem -> setupTimeStepping -> advanceInTime
// with "Class" = "Newmark" (DAESolverInTime::advanceInTimeLinearNewmark, DAESolverInTime_def.hpp:519-607).  Mesh choice, command
// line and output follow linelas_main.cpp: the structured square / cube with "H/h" cells per direction (the reference reads an
// unstructured mesh file here), the displacement after the last step as text, ParaView export per step when the settings ask.
#include <chrono>
#include <cmath>
#include <cstring>
#include <fstream>
#include <iomanip>

#include "feddlib/core/FEDDCore.hpp"
#include "feddlib/core/FE/Domain.hpp"
#include "feddlib/core/General/BCBuilder.hpp"
#include "feddlib/core/General/ExporterParaView.hpp"
#include "feddlib/problems/Solver/DAESolverInTime.hpp"
#include "feddlib/problems/specific/LinElas.hpp"

// the reference's load functions: parameters[0] is the time, parameters[1] the volume force; the load is switched off after
// t = 1 (2D) / t = 0.2 (3D)
void rhs2D(double* x, double* res, double* parameters) {
    res[0] = 0.;
    res[1] = 0.;
    if (parameters[0] <= 1.) res[1] = parameters[1];
}
void rhs(double* x, double* res, double* parameters) {
    res[0] = 0.;
    res[1] = 0.;
    if (parameters[0] <= 0.2) res[1] = parameters[1];
    res[2] = 0.;
}
void zeroDirichlet2D(double* x, double* res, double t, const double* parameters) { res[0] = 0.; res[1] = 0.; }
void zeroDirichlet3D(double* x, double* res, double t, const double* parameters) { res[0] = 0.; res[1] = 0.; res[2] = 0.; }

typedef default_sc SC;
typedef default_lo LO;
typedef default_go GO;
typedef default_no NO;

using namespace FEDD;

int main(int argc, char* argv[]) {
    Teuchos::GlobalMPISession mpiSession(&argc, &argv);
    std::string xmlProblemFile = "parametersProblem.xml", xmlPrecFile = "parametersPrec.xml", xmlSolverFile = "parametersSolver.xml";
    std::string outFile = "solutionUnsteadyLinElas.txt";
    for (int i = 1; i < argc; ++i) {
        std::string a(argv[i]);
        auto val = [&](const char* key, std::string& dst) {
            const std::string k = std::string("--") + key + "=";
            if (a.compare(0, k.size(), k) == 0) { dst = a.substr(k.size()); return true; }
            return false;
        };
        if (val("problemfile", xmlProblemFile) || val("precfile", xmlPrecFile) || val("solverfile", xmlSolverFile) || val("out", outFile)) continue;
        std::cerr << "unknown option " << a << std::endl;
        return 2;
    }
    try {
        Teuchos::RCP<const Teuchos::Comm<int> > comm = Teuchos::DefaultComm<int>::getComm();
        const bool verbose = comm->getRank() == 0;
        ParameterListPtr_Type parameterListProblem = Teuchos::getParametersFromXmlFile(xmlProblemFile);
        ParameterListPtr_Type parameterListPrec = Teuchos::getParametersFromXmlFile(xmlPrecFile);
        ParameterListPtr_Type parameterListSolver = Teuchos::getParametersFromXmlFile(xmlSolverFile);
        ParameterListPtr_Type parameterListAll(new Teuchos::ParameterList(*parameterListProblem));
        parameterListAll->setParameters(*parameterListPrec);
        parameterListAll->setParameters(*parameterListSolver);

        int dim = parameterListProblem->sublist("Parameter").get("Dimension", 2);
        int m = parameterListProblem->sublist("Parameter").get("H/h", 5);
        int zeroDirID = parameterListProblem->sublist("Parameter").get("Homogeneous Dirichlet Flag", 1);
        std::string discType = parameterListProblem->sublist("Parameter").get("Discretization", "P2");
        std::string bcType = parameterListProblem->sublist("Parameter").get("BC Type", "volumeY");

        Teuchos::RCP<Domain<SC, LO, GO, NO> > domain;
        if (dim == 2) {
            std::vector<double> x(2, 0.0);
            domain = Teuchos::rcp(new Domain<SC, LO, GO, NO>(x, 1., 1., comm));
        } else {
            std::vector<double> x(3, 0.0);
            domain = Teuchos::rcp(new Domain<SC, LO, GO, NO>(x, 1., 1., 1., comm));
        }
        domain->buildMesh(1, "Square", dim, discType, 1, m, 0);

        Teuchos::RCP<BCBuilder<SC, LO, GO, NO> > bcFactory(new BCBuilder<SC, LO, GO, NO>());
        bcFactory->addBC(dim == 2 ? zeroDirichlet2D : zeroDirichlet3D, zeroDirID, 0, domain, "Dirichlet", dim);

        LinElas<SC, LO, GO, NO> linElas(domain, discType, parameterListAll);
        domain->info();
        linElas.info();
        TEUCHOS_TEST_FOR_EXCEPTION(bcType != "volumeY", std::runtime_error, "Unknown boundary function.");
        linElas.addRhsFunction(dim == 2 ? rhs2D : rhs);
        double force = parameterListAll->sublist("Parameter").get("Volume force", 0.);
        double finalTimeRamp = parameterListAll->sublist("Timestepping Parameter").get("Final time force", 0.1);
        double degree = 0;
        linElas.addParemeterRhs(force);
        linElas.addParemeterRhs(finalTimeRamp);
        linElas.addParemeterRhs(degree);

        const auto t0 = std::chrono::steady_clock::now();
        linElas.addBoundaries(bcFactory);
        linElas.initializeProblem();
        linElas.assemble();

        DAESolverInTime<SC, LO, GO, NO> daeTimeSolver(parameterListAll, comm);
        SmallMatrix<int> defTS(1);
        defTS[0][0] = 1;
        daeTimeSolver.defineTimeStepping(defTS);
        daeTimeSolver.setProblem(linElas);
        daeTimeSolver.setupTimeStepping();
        daeTimeSolver.advanceInTime();
        const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (verbose) {
            std::cout << "time steps " << daeTimeSolver.stepsDone() << " combines " << daeTimeSolver.getTimeProblem()->numberOfCombines()
                      << " relres " << daeTimeSolver.getTimeProblem()->getLastRelativeResidual() << std::endl;
            std::cout << "Solve Problem " << secs << " s" << std::endl;
        }
        Teuchos::RCP<const MultiVector<SC, LO, GO, NO> > exportSolution = linElas.getSolution()->getBlock(0);
        std::ofstream out(outFile);
        out << std::setprecision(17);
        auto map = exportSolution->getMap();
        auto data = exportSolution->getData(0);
        for (size_t i = 0; i < data.size(); ++i) out << map->getGlobalElement((LO)i) << " " << data[i] << "\n";
    } catch (const std::exception& e) {
        std::cerr << "exception: " << e.what() << std::endl;
        return 1;
    }
    return 0;
}
